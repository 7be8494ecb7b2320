"""Per-group learning rates on the parameter arena, on the GPU: dn_sgd_step_groups against dn_sgd_step run by run (bit for bit), FusedSGD
with two groups against torch.optim.SGD, one group against the flat form, rates changed between steps, a bucket at a time under the
backward pass, on the launch tape with BatchNorm frozen, across a checkpoint, and from train.py's command line (--diff-lr)."""
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
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import bench  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
from supervised_dispnet_amd import _lib, engine  # noqa: E402
from supervised_dispnet_amd.functional import reciprocal  # noqa: E402
from supervised_dispnet_amd.optim import FusedSGD  # noqa: E402
from test_gpu_sgd import SHAPES, _buffer_of, _grad, _run_train, close  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 12345.0
RATES = [1e-2, 1e-1, 3e-3]
MOMENTUM, WD, SCALE = 0.9, 5e-4, 0.5


# ------------------------------------------------------------------------------------------------ 1. the kernel, through the C ABI
def _tiny_runs():
    """700 runs of 4, 8 or 12 elements alternating between two groups."""
    gen = torch.Generator().manual_seed(11)
    lengths = (4 * torch.randint(1, 4, (700,), generator=gen)).tolist()
    lengths[340], lengths[20], lengths[680] = 12, 8, 8                   # (whatever the draw, the ranges below find their runs)
    return np.cumsum(lengths).tolist(), [i % 2 for i in range(700)]


def _layouts():
    big = 4194304 + 4116
    ends_c, groups_c = _tiny_runs()
    s = lambda ends, r: ends[r - 1] if r else 0                          # start of run r
    return {
        # name: (ends, groups, [whole range, a range from the middle of one run to the middle of another, a range inside one run])
        "a-44": ([4, 8, 24, 44], [0, 1, 0, 2], [(0, 44), (12, 32), (28, 40)]),
        "b-wave-and-block-edges": ([252, 256, 260, 1024, 1028, 5000], [0, 1, 2, 0, 1, 2], [(0, 5000), (128, 3000), (1100, 4900)]),
        "c-700-runs": (ends_c, groups_c, [(0, ends_c[-1]), (s(ends_c, 20) + 4, ends_c[680] - 4), (s(ends_c, 340) + 4, s(ends_c, 340) + 8)]),
        "d-second-pass": ([4, 4194300, 4194312, big], [0, 1, 0, 1], [(0, big), (2048, 4194304 + 2000), (4194320, big - 420)]),
    }


LAYOUTS = _layouts()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_grouped_kernel_is_bitwise_dn_sgd_step_run_by_run(layout):
    """Two consecutive dn_sgd_step_groups launches over [lo, hi) against dn_sgd_step on every (run, range) intersection with that run's
    group's rate: torch.equal on p and the momentum buffer, sentinels outside the range untouched, the gradient unmodified."""
    ends, groups, ranges = LAYOUTS[layout]
    n = ends[-1]
    assert all(e % 4 == 0 for e in ends) and ends == sorted(set(ends)) and len(ends) == len(groups)
    gen = torch.Generator().manual_seed(n)
    vals = [torch.randn(n, generator=gen).to(DEV) for _ in range(3)]
    seg_end = torch.tensor(ends, dtype=torch.int64, device=DEV)
    seg_group = torch.tensor(groups, dtype=torch.int32, device=DEV)
    rates = torch.tensor(RATES, dtype=torch.float64, device=DEV)
    s = engine._stream()
    starts = [0] + ends[:-1]
    for lo, hi in ranges:
        assert 0 <= lo < hi <= n and lo % 4 == 0 and hi % 4 == 0
        inside = torch.zeros(n, dtype=torch.bool, device=DEV)
        inside[lo:hi] = True

        def fresh():
            p, g, b = (v.clone() for v in vals)
            p[~inside] = SENTINEL
            b[~inside] = SENTINEL
            assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            return p, g, b

        p, g, b = fresh()
        for _ in range(2):                                             # the second step reads the buffer the first one wrote
            _lib.call("dn_sgd_step_groups", p.data_ptr(), g.data_ptr(), b.data_ptr(), lo, hi, seg_end.data_ptr(), seg_group.data_ptr(),
                      len(ends), rates.data_ptr(), len(RATES), MOMENTUM, WD, SCALE, s)
        wp, wg, wb = fresh()
        touched = 0
        for a, e, grp in zip(starts, ends, groups):
            a, e = max(a, lo), min(e, hi)
            if a < e:
                touched += 1
                for _ in range(2):
                    _lib.call("dn_sgd_step", wp.data_ptr() + 4 * a, wg.data_ptr() + 4 * a, wb.data_ptr() + 4 * a, e - a, RATES[grp], MOMENTUM,
                              WD, SCALE, s)
        assert touched >= 1
        assert torch.equal(p, wp), (layout, lo, hi, int((p != wp).sum()))
        assert torch.equal(b, wb), (layout, lo, hi, int((b != wb).sum()))
        assert torch.equal(g, vals[1]) and torch.equal(wg, vals[1])
        assert bool((p[~inside] == SENTINEL).all()) and bool((b[~inside] == SENTINEL).all())
        assert not torch.equal(p[lo:hi], vals[0][lo:hi]) and not torch.equal(b[lo:hi], vals[2][lo:hi])


def test_grouped_kernel_refuses_bad_arguments():
    t = torch.zeros(64, device=DEV)
    se = torch.tensor([64], dtype=torch.int64, device=DEV)
    sg = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr = torch.tensor([0.1], dtype=torch.float64, device=DEV)
    p, s = t.data_ptr(), engine._stream()
    E, G, L = se.data_ptr(), sg.data_ptr(), lr.data_ptr()
    assert p % 16 == 0
    good = (p, p, p, 0, 64, E, G, 1, L, 1)
    bad = [(0, p, p, 0, 64, E, G, 1, L, 1), (p, 0, p, 0, 64, E, G, 1, L, 1), (p, p, 0, 0, 64, E, G, 1, L, 1),          # null pointers
           (p, p, p, 0, 64, 0, G, 1, L, 1), (p, p, p, 0, 64, E, 0, 1, L, 1), (p, p, p, 0, 64, E, G, 1, 0, 1),
           (p, p, p, 8, 8, E, G, 1, L, 1), (p, p, p, 16, 8, E, G, 1, L, 1), (p, p, p, -4, 8, E, G, 1, L, 1),           # hi <= lo, lo < 0
           (p + 4, p, p, 0, 32, E, G, 1, L, 1), (p, p + 8, p, 0, 32, E, G, 1, L, 1), (p, p, p + 4, 0, 32, E, G, 1, L, 1),   # misaligned bases
           (p, p, p, 2, 64, E, G, 1, L, 1), (p, p, p, 0, 62, E, G, 1, L, 1),                                           # ... and offsets
           (p, p, p, 0, 64, E, G, 0, L, 1), (p, p, p, 0, 64, E, G, -1, L, 1), (p, p, p, 0, 64, E, G, 1, L, 0)]         # n_seg, n_groups < 1
    assert all(len(a) == len(good) for a in bad)
    for args in bad:
        with pytest.raises(_lib.DispnetHipError, match="dn_sgd_step_groups: bad argument"):
            _lib.call("dn_sgd_step_groups", *args, 0.9, 0.0, 1.0, s)
    torch.cuda.synchronize()
    assert not bool(t.any())


# ------------------------------------------------------------------------------------------------ 2.-4. the optimizer
def _alternating(ps, rates=(1e-2, 1e-1)):
    return [{"params": ps[0::2], "lr": rates[0]}, {"params": ps[1::2], "lr": rates[1]}]


@pytest.mark.parametrize("momentum,wd", [(0.9, 0.0), (0.9, 5e-4), (0.0, 5e-4), (0.0, 0.0)])
def test_two_groups_match_torch_sgd_with_two_groups(momentum, wd):
    torch.manual_seed(0)
    ref_p = [torch.randn(s).requires_grad_() for s in SHAPES]
    dev_p = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    opt_ref = torch.optim.SGD(_alternating(ref_p), lr=1.0, momentum=momentum, weight_decay=wd)
    opt = FusedSGD(_alternating(dev_p), momentum=momentum, weight_decay=wd, production_order=dev_p)
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 1e-1] == [g["lr"] for g in opt_ref.param_groups]
    assert [[id(p) for p in g["params"]] for g in opt.param_groups] == [[id(p) for p in dev_p[0::2]], [id(p) for p in dev_p[1::2]]]
    for g in opt.param_groups:
        assert (g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"]) == (momentum, wd, 0, False)
    assert opt.arena.runs == [(1728, 0), (1792, 1), (1812, 0), (75540, 1), (75684, 0)]       # alternating on every slice; (17,) padded
    for it in range(3):
        for p, q in zip(ref_p, dev_p):
            gr = _grad(p, it)
            p.grad = gr.clone()
            q._dn_grad_view.copy_(gr.to(DEV))
        opt_ref.step()
        opt.step()
        for p, q in zip(ref_p, dev_p):
            close("grouped sgd p, step %d" % it, q.detach(), p.detach())
    for p, q in zip(ref_p, dev_p):
        if momentum != 0:
            close("grouped sgd momentum_buffer", _buffer_of(opt, q), opt_ref.state[p]["momentum_buffer"])
    pad = torch.ones(opt.arena.numel, dtype=torch.bool, device=DEV)
    for q, o in zip(opt.arena.params, opt.arena.offsets):
        pad[o:o + q.numel()] = False
    assert int(pad.sum()) == 3 and not bool(opt.momentum_buffer[pad].any()) and not bool(opt.arena.flat_p[pad].any())


def _two_optimizers(make_a, make_b, seed=1):
    torch.manual_seed(seed)
    init = [torch.randn(s) for s in SHAPES]
    out = []
    for make in (make_a, make_b):
        ps = [nn.Parameter(p.clone().to(DEV)) for p in init]
        out.append((ps, make(ps)))
    return out


def _steps(opts, its, scale=0.5):
    for it in its:
        for ps, o in opts:
            for q in ps:
                q._dn_grad_view.copy_(_grad(q, it % 3).to(DEV))
            o.step(grad_scale=scale)
        (_, a), (_, b) = opts
        assert torch.equal(a.arena.flat_p, b.arena.flat_p), it
        assert torch.equal(a.momentum_buffer, b.momentum_buffer), it


def test_one_group_as_a_dict_is_the_flat_optimizer():
    lr = 1e-2
    opts = _two_optimizers(lambda ps: FusedSGD(ps, lr=lr, momentum=0.9, weight_decay=5e-4),
                           lambda ps: FusedSGD([{"params": ps, "lr": lr}], momentum=0.9, weight_decay=5e-4))
    (_, flat), (_, one) = opts
    assert one._table is None and flat._table is None
    assert len(one.param_groups) == 1 and list(one.param_groups[0]) == list(flat.param_groups[0])
    assert {k: v for k, v in one.param_groups[0].items() if k != "params"} == {k: v for k, v in flat.param_groups[0].items() if k != "params"}
    assert [id(p) for p in one.param_groups[0]["params"]] == [id(p) for p in one.arena.params]
    _steps(opts, range(3))
    sa, sb = flat.state_dict(), one.state_dict()
    assert set(sa) == set(sb) == {"momentum_buffer", "param_groups"} and sa["param_groups"] == sb["param_groups"]
    assert sb["param_groups"] == [{"lr": lr, "momentum": 0.9, "weight_decay": 5e-4, "dampening": 0, "nesterov": False}]
    one.capturable(True)
    assert one._dev is not None                                        # (and the device-side form of today)


def test_rates_follow_set_lr_and_param_group_writes_and_capturable_changes_nothing():
    make = lambda on: (lambda ps: FusedSGD(_alternating(ps), momentum=0.9, weight_decay=5e-4, production_order=ps).capturable(on))
    opts = _two_optimizers(make(False), make(True))
    (ps_h, opt_h), (_, opt_d) = opts
    for o in (opt_h, opt_d):
        assert len(o.arena.runs) == 5 and o._dev is None and o._table["lr"].dtype == torch.float64 and o._table["lr"].tolist() == [1e-2, 1e-1]
        assert [t.data_ptr() for t in o.tape_state()] == [o.arena.flat_p.data_ptr(), o.momentum_buffer.data_ptr()]
    _steps(opts, range(2))
    for _, o in opts:                                                   # a scheduler, through set_lr
        o.set_lr(3e-3, group=1)
        assert o._table["lr"].tolist() == [1e-2, 3e-3] and o.param_groups[1]["lr"] == 3e-3
    before = opt_h.arena.flat_p.clone()
    _steps(opts, range(2, 4))
    for _, o in opts:                                                   # ... and one that writes the parameter group as torch's do
        o.param_groups[0]["lr"] = 7e-4
        o.param_groups[1]["lr"] = 5e-2
    _steps(opts, range(4, 6))
    assert opt_d._table["lr"].tolist() == [7e-4, 5e-2]
    # the changed rates are what moved the parameters: an optimizer left at the first rates ends elsewhere, in both groups
    ref = _two_optimizers(make(False), make(False))
    _steps(ref, range(6))
    stale = ref[0][1]
    for q, r in zip(ps_h, ref[0][0]):
        assert not torch.equal(q.detach(), r.detach())
    assert not torch.equal(before, stale.arena.flat_p)
    # set_lr on group 0 is the default
    opt_h.set_lr(1e-5)
    assert opt_h._table["lr"].tolist() == [1e-5, 5e-2]


# ------------------------------------------------------------------------------------------------ 5.-6. under the backward pass, on the tape
def _make(sd0=None, freeze=False, rates=(1e-4, 1e-3)):
    import train
    torch.manual_seed(0)
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    bench._quiet_init(net)
    if sd0 is not None:
        net.load_state_dict(sd0)
    net.to(DEV).train()
    if freeze:
        assert train.freeze_batchnorm(net) == 13
    groups = train.diff_lr_groups(net, rates[0])
    assert [g["lr"] for g in groups] == [rates[0], 10 * rates[0]]
    groups[1]["lr"] = rates[1]
    opt = FusedSGD(groups, momentum=0.9, weight_decay=5e-4, production_order=net._grad_production_order())
    assert len(opt.arena.runs) == 2 and opt._table is not None
    return net, opt


def _state_equal(net_a, net_b):
    sa, sb = net_a.state_dict(), net_b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("taped", [False, True], ids=["eager", "taped"])
def test_groups_per_bucket_under_the_backward_pass_are_bitwise_the_whole_arena_step(taped):
    from supervised_dispnet_amd.distributed import GradReducer
    from supervised_dispnet_amd.graph import TapedStep, backward
    batches = [bench.synthetic_batch(4, 64, 96, DEV, seed) for seed in range(4)]
    net_a, opt_a = _make()
    sd0 = copy.deepcopy({k: v.detach().cpu().clone() for k, v in net_a.state_dict().items()})
    net_b, opt_b = _make(sd0)
    red = GradReducer(opt_b.arena, bucket_bytes=8 << 20, comm="torch")
    assert red.path == "none" and len(red.buckets) >= 4
    # buckets end on parameter boundaries, so they begin and end in the middle of runs, and both runs are cut into several buckets
    bounds = {0} | {e for e, _ in opt_b.arena.runs}
    assert sum(1 for b in red.buckets if b["lo"] not in bounds or b["hi"] not in bounds) >= 4
    edge = opt_b.arena.runs[0][0]
    assert sum(1 for b in red.buckets if b["hi"] <= edge) >= 2 and sum(1 for b in red.buckets if b["lo"] >= edge) >= 2
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
    if taped:
        f.close()


def test_launch_tape_replay_with_frozen_batchnorm_is_bitwise_the_eager_grouped_step():
    from supervised_dispnet_amd.graph import TapedStep, backward
    batches = [bench.synthetic_batch(2, 64, 96, DEV, seed) for seed in range(6)]
    net_e, opt_e = _make(freeze=True)
    sd0 = copy.deepcopy({k: v.detach().cpu().clone() for k, v in net_e.state_dict().items()})
    net_t, opt_t = _make(sd0, freeze=True)
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

    ts = TapedStep(step_t, optimizer=opt_t, warmup=1, static_inputs=(img, gt))
    ts.capture()                       # one warm-up step + the recorded one: two real steps on batch 0
    for _ in range(2):
        step_e(*batches[0])
    assert ts.launches > 100 and ts.segments == 1

    def replay_and_compare(some):
        for x, y in some:
            img.copy_(x)
            gt.copy_(y)
            lt = ts().clone()
            le = step_e(x, y).clone()
            assert torch.isfinite(lt).all() and torch.equal(lt, le), (lt, le)
        torch.cuda.synchronize()
        assert torch.equal(opt_t.arena.flat_p, opt_e.arena.flat_p)
        assert torch.equal(opt_t.momentum_buffer, opt_e.momentum_buffer)

    replay_and_compare(batches[1:3])
    for o in (opt_t, opt_e):           # a scheduler between replays: the tape reads the rate from the device table
        o.set_lr(2e-5, group=0)
    replay_and_compare(batches[3:5])
    for o in (opt_t, opt_e):
        o.set_lr(4e-4, group=1)
    replay_and_compare(batches[5:])
    _state_equal(net_t, net_e)
    for k, v in net_t.state_dict().items():                             # frozen: the running statistics never moved
        if k.endswith("running_mean"):
            assert not bool(v.any()), k
        if k.endswith("running_var"):
            assert bool((v == 1).all()), k
    ts.close()


# ------------------------------------------------------------------------------------------------ 7. checkpoints
def test_resume_from_own_and_from_two_group_torch_sgd_state():
    torch.manual_seed(2)
    momentum, wd = 0.9, 5e-4
    ref_p = [torch.randn(s).requires_grad_() for s in SHAPES]
    dev_p = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    opt_ref = torch.optim.SGD(_alternating(ref_p), lr=1.0, momentum=momentum, weight_decay=wd)
    opt = FusedSGD(_alternating(dev_p), momentum=momentum, weight_decay=wd, production_order=dev_p)

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
    # (a) the own form: each group's hyper-parameters plus torch's construction-order indices
    sd = opt.state_dict()
    assert set(sd) == {"momentum_buffer", "param_groups"} and sd["momentum_buffer"].shape == (opt.arena.numel,)
    assert sd["param_groups"] == [{"lr": 1e-2, "momentum": momentum, "weight_decay": wd, "dampening": 0, "nesterov": False, "params": [0, 1, 2]},
                                  {"lr": 1e-1, "momentum": momentum, "weight_decay": wd, "dampening": 0, "nesterov": False, "params": [3, 4]}]
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in opt_ref.state_dict()["param_groups"]]
    new_p = [nn.Parameter(q.detach().clone()) for q in dev_p]
    opt2 = FusedSGD(_alternating(new_p), momentum=momentum, weight_decay=wd, production_order=new_p)
    opt2.load_state_dict(sd)
    # (b) torch.optim.SGD's two-group state after the same two steps on the CPU, into an arena that orders the parameters differently
    tp = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    opt3 = FusedSGD(_alternating(tp), momentum=momentum, weight_decay=wd, production_order=[tp[i] for i in (3, 0, 4, 2, 1)])
    assert [id(p) for p in opt3.arena.params] == [id(tp[i]) for i in (3, 0, 4, 2, 1)] and opt3.arena.group_of == [1, 0, 0, 0, 1]
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
    # (c) another grouping is refused, whichever form it comes in, and leaves the buffer alone
    kept = opt2.momentum_buffer.clone()
    other = torch.optim.SGD([{"params": ref_p[:2], "lr": 1e-2}, {"params": ref_p[2:], "lr": 1e-1}], lr=1.0, momentum=momentum)
    flat_sd = FusedSGD([nn.Parameter(q.detach().clone()) for q in dev_p], lr=1e-2, momentum=momentum, weight_decay=wd).state_dict()
    moved = dict(sd, param_groups=[dict(sd["param_groups"][0], params=[0, 1]), dict(sd["param_groups"][1], params=[2, 3, 4])])
    for bad in (other.state_dict(), flat_sd, moved, torch.optim.SGD(ref_p, lr=1e-2, momentum=momentum).state_dict()):
        with pytest.raises(ValueError, match=r"this optimizer has groups of sizes \[3, 2\]"):
            opt2.load_state_dict(bad)
    with pytest.raises(ValueError, match="arena has"):
        opt2.load_state_dict(dict(sd, momentum_buffer=torch.zeros(8)))
    assert torch.equal(opt2.momentum_buffer, kept)
    flat = FusedSGD([nn.Parameter(q.detach().clone()) for q in dev_p], lr=1e-2, momentum=momentum, weight_decay=wd)
    with pytest.raises(ValueError, match=r"groups of sizes \[3, 2\], this optimizer has groups of sizes \[5\]"):
        flat.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_train_cli_diff_lr_on_the_launch_tape_equals_the_eager_run(tmp_path, capsys):
    args = ["--network", "disp_vgg_BN", "--with-gt", "--loss", "L1", "--diff-lr", "--seed", "3"]
    ve, sde, _ = _run_train(tmp_path / "eager", args + ["--no-tape"])
    out = capsys.readouterr().out
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    n1, n10 = len(list(net.get_1x_lr_params())), len(list(net.get_10x_lr_params()))
    line = "=> setting sgd solver with two learning rates: {} parameters at 0.001 (encoder), {} at 0.01".format(n1, n10)
    assert line in out and "--tape:" not in out, out[-600:]
    vt, sdt, ckpt = _run_train(tmp_path / "tape", args)                                  # (no flag: the tape is the default)
    out = capsys.readouterr().out
    assert line in out and "=> setting adam solver" not in out
    assert "--tape:" in out and "bit for bit" in out, out[-600:]
    assert "eager launches (" not in out
    assert vt.shape == ve.shape and np.array_equal(vt, ve), (vt[:, 0], ve[:, 0])
    for k, v in sde["state_dict"].items():
        assert torch.equal(v, sdt["state_dict"][k]), k
    groups = sdt["optimizer"]["param_groups"]
    assert [g["lr"] for g in groups] == [1e-3, 1e-2] and [len(g["params"]) for g in groups] == [n1, n10]
    assert sorted(groups[0]["params"] + groups[1]["params"]) == list(range(n1 + n10))
    mb = sdt["optimizer"]["momentum_buffer"]
    assert mb.dim() == 1 and bool(mb.any()) and torch.equal(mb, sde["optimizer"]["momentum_buffer"])
    assert mb.numel() == sum((p.numel() + 3) // 4 * 4 for p in net._hot_parameters())
    fresh = net.state_dict()
    stats = [k for k in fresh if "running_" in k or k.endswith("num_batches_tracked")]
    assert len(stats) == 3 * 13
    for k in stats:                                                     # BatchNorm is frozen: the running statistics are the initial ones
        assert torch.equal(sdt["state_dict"][k], fresh[k]), k
    _run_train(tmp_path / "resumed", args + ["--pretrained-disp", ckpt], epochs=1, n=4)
    out = capsys.readouterr().out
    assert line in out and "not restored" not in out


def test_train_cli_diff_lr_on_a_resnet_and_with_the_dorn_head(tmp_path, capsys):
    _run_train(tmp_path / "res18", ["--network", "disp_res_18", "--with-gt", "--loss", "L1", "--diff-lr", "--seed", "3"], epochs=1)
    out = capsys.readouterr().out
    assert "=> setting sgd solver with two learning rates" in out and "eager launches (" not in out
    _vals, sd, _ = _run_train(tmp_path / "dorn", ["--network", "disp_vgg_BN_DORN", "--loss", "DORN", "--ordinal-c", "16", "--with-gt", "--diff-lr",
                                                 "--seed", "3", "--tape"], epochs=1)
    out = capsys.readouterr().out
    assert "=> setting sgd solver with two learning rates" in out
    assert "=> --tape: eager launches (only the supervised depth losses are taped)" in out          # the DORN run is eager and says so
    assert len(sd["optimizer"]["param_groups"]) == 2


def test_train_cli_diff_lr_without_a_pretrainable_encoder_keeps_its_exit(tmp_path):
    import train
    with pytest.raises(SystemExit, match=r"--diff-lr needs a network with get_1x_lr_params\(\) / get_10x_lr_params\(\) \(reference: models.DORN only\)"):
        train.main(["SYN", "--synthetic", "8", "-b", "4", "--epochs", "1", "--img-height", "64", "--img-width", "96", "--save-root", str(tmp_path),
                    "--network", "dispnet", "--with-gt", "--loss", "L1", "--diff-lr"])
