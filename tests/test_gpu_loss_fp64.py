"""The supervised-loss, ordinal and error-metric kernels (csrc/dn_loss.hip, csrc/dn_ordinal.hip) against the fp64 oracle, on the cases
of tests/loss_audit.py: every split regime of the masked forward, the 256 / 257 group boundary of its fused form, the second trip of the
backward grid, the clamp and validity edges, berHu ties, four terms of different size accumulated into one scalar, the minimum sizes of
the integer upsample, the clamps of the explainability loss, the ordinal head in both layouts, the DORN loss around its 8-plane
unroll, SID labels at the bin edges and compute_errors with its radix-select median.  pytest -m gpu.

Every tolerance is loss_audit.check() (geom_audit's): MARGIN x the fp32 CPU oracle's own error against fp64 on the same inputs,
fragile elements handled beforehand (tests/test_loss_audit_host.py shows what that rejects).  Each comparison prints its figures; the
worst per quantity are recorded in loss_audit's docstring.  The cases run through the public functions of loss_functions.py / utils.py
/ the OrdinalRegressionLayer; only the medians (which compute_errors does not return) and the argument checks use the raw entry points.
Which forward a masked loss took is read from the entry point that loss_functions handed to engine.hbm_call (dn_last_kernel() names
conv-family kernels only).
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

import loss_audit as LA  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.utils as UT  # noqa: E402
from supervised_dispnet_amd import _lib  # noqa: E402
from supervised_dispnet_amd.models.Disp_vgg_BN_DORN import OrdinalRegressionLayer  # noqa: E402

DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
DN_ERR_BAD_ARG, DN_ERR_WORKSPACE = -1, -3
PER_SAMPLE = {"l1": LF.l1_loss, "l2": LF.l2_loss, "berhu": LF.berhu_loss, "scale_inv": LF.Scale_invariant_loss}


def dev(t):
    return t.to(DEV)


def zeros_kept(got, ref64):
    """where the fp64 gradient is exactly 0 (an invalid pixel, a prediction outside the clamp, d == 0) the kernel's is exactly 0 too"""
    return float(got.detach().cpu()[ref64 == 0].abs().sum()) == 0.0


def bits_equal(a, b):
    """equal bit patterns (NaN included)"""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture
def forward_path(monkeypatch):
    """run(fused, fn) -> (fn(), the masked-forward entry points it went through)"""
    calls = []
    real = LF.hbm_call

    def spy(kernel, nbytes, entry, *args):
        if entry.startswith("dn_masked_loss_fwd"):
            calls.append(entry)
        return real(kernel, nbytes, entry, *args)

    monkeypatch.setattr(LF, "hbm_call", spy)

    def run(fused, fn):
        monkeypatch.setattr(LF, "FUSE_MASKED_FWD", fused)
        del calls[:]
        out = fn()
        torch.cuda.synchronize()
        return out, list(calls)

    return run


# ------------------------------------------------------------------------------------------------------ per-sample losses
def _per_sample(name, kind):
    gt, pred = LA.masked_inputs(name)
    p = dev(pred).requires_grad_()
    v = PER_SAMPLE[kind](dev(gt), [p], "kitti")
    v.backward()
    return v.detach(), p.grad


@pytest.mark.parametrize("name", list(LA.MASKED_CASES))
def test_per_sample_losses_vs_fp64(name, forward_path):
    groups = LA.MASKED_CASES[name][0]
    for kind in LA.KINDS:
        if name in ("berhu_ties", "berhu_flat") and kind != "berhu":
            continue
        (l64, g64), (l32, g32) = LA.per_sample_reference(name, kind, F64), LA.per_sample_reference(name, kind, F32)
        got = {}
        for fused in (True, False):
            got[fused], entries = forward_path(fused, lambda: _per_sample(name, kind))
            takes_fused = fused and kind != "berhu" and groups <= LA.FOLD_GROUPS
            assert entries == ["dn_masked_loss_fwd_fused" if takes_fused else "dn_masked_loss_fwd"], (name, kind, fused, entries)
            again, _ = forward_path(fused, lambda: _per_sample(name, kind))
            assert bits_equal(again[0], got[fused][0]) and bits_equal(again[1], got[fused][1]), "%s %s: two runs differ" % (name, kind)
            loss, dpred = got[fused]
            tag = "%s:%s:%s" % (name, kind, "fused" if fused else "three")
            if name == "empty_group":       # NaN by design; the empty sample gets no gradient, the others theirs
                assert bool(torch.isnan(loss)) and bool(torch.isnan(l64))
                assert float(dpred[1].abs().max()) == 0.0
            elif name == "berhu_flat":      # max r == 0: the loss and every gradient are exactly 0
                assert float(loss) == 0.0 and float(dpred.abs().max()) == 0.0
                continue
            elif name != "bwd_grid_cap":
                LA.check(tag + ":loss", loss, l64, l32)
            LA.check(tag + ":dpred", dpred, g64, g32)
            assert zeros_kept(dpred, g64), tag
        if kind != "berhu":
            assert bits_equal(got[True][0], got[False][0]) and bits_equal(got[True][1], got[False][1]), \
                "%s %s: the fused forward and the three launches differ" % (name, kind)


# ------------------------------------------------------------------------------------------------------------ multiscale
def _multiscale(fn, pool):
    gt, preds = LA.multiscale_inputs()
    ps = [dev(p).requires_grad_() for p in preds]
    f = getattr(LF, fn)
    v = f(dev(gt), ps, pool) if pool else f(dev(gt), ps)
    v.backward()
    return v.detach(), [p.grad for p in ps]


def test_pyramids_of_the_multiscale_case_are_exact():
    gt, _ = LA.multiscale_inputs()
    for pool in ("max", "avg", "bilinear"):
        ours = getattr(LF, "generate_%s_pyramid" % pool)(dev(gt))
        for a, b in zip(ours, LA.OL._gt_pyramid(gt.double(), pool)):
            assert torch.equal(a.cpu().double(), b.reshape(a.shape))


@pytest.mark.parametrize("run", LA.MULTISCALE_RUNS, ids=lambda r: "%s-%s" % (r[0], r[1]))
def test_multiscale_losses_vs_fp64(run, forward_path):
    fn, pool, kind = run
    r64, r32 = LA.multiscale_reference(fn, pool, kind, F64), LA.multiscale_reference(fn, pool, kind, F32)
    got = {}
    for fused in (True, False):
        got[fused], entries = forward_path(fused, lambda: _multiscale(fn, pool))
        assert entries == ["dn_masked_loss_fwd_fused" if fused and kind != "berhu" else "dn_masked_loss_fwd"] * 4
        again, _ = forward_path(fused, lambda: _multiscale(fn, pool))
        assert bits_equal(again[0], got[fused][0]) and all(bits_equal(a, b) for a, b in zip(again[1], got[fused][1]))
        tag = "%s:%s:%s" % (fn, pool, "fused" if fused else "three")
        LA.check(tag + ":loss", got[fused][0], r64[0], r32[0])
        for i in range(4):
            LA.check(tag + ":dpred%d" % i, got[fused][1][i], r64[1][i], r32[1][i])
            # (under the bilinear upsample a zero of the fp64 gradient is a cancellation of +-w / n terms with dyadic w, not a structural zero)
            assert (fn, pool) == ("Multiscale_FULL_L1_loss", "bilinear") or zeros_kept(got[fused][1][i], r64[1][i]), tag
    if kind != "berhu":
        assert bits_equal(got[True][0], got[False][0]) and all(bits_equal(a, b) for a, b in zip(got[True][1], got[False][1]))


# -------------------------------------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("mode", LA.UPSAMPLE["modes"])
def test_upsample_min_vs_fp64(mode):
    for size in LA.UPSAMPLE["sizes"]:
        for scale in LA.UPSAMPLE["scales"]:
            x, g = LA.upsample_inputs(size, scale)
            r64, r32 = LA.upsample_reference(size, scale, mode, F64), LA.upsample_reference(size, scale, mode, F32)
            outs = []
            for _ in range(2):
                xl = dev(x).requires_grad_()
                out = LF._UpsampleInt.apply(xl, scale, 0 if mode == "nearest" else 1)
                (out * dev(g)).sum().backward()
                torch.cuda.synchronize()
                outs.append((out.detach(), xl.grad))
            assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])
            tag = "upsample:%s:%dx%d:x%d" % ((mode,) + size + (scale,))
            LA.check(tag + ":out", outs[0][0], r64[0], r32[0])
            LA.check(tag + ":dx", outs[0][1], r64[1], r32[1])


# -------------------------------------------------------------------------------------------------------- explainability
@pytest.mark.parametrize("n", LA.EXPLAIN_SIZES)
def test_explainability_edges_vs_fp64(n):
    m, edge = LA.explain_inputs(n)
    r64, r32 = LA.explain_reference(n, F64), LA.explain_reference(n, F32)
    outs = []
    for _ in range(2):
        ml = dev(m).requires_grad_()
        v = LF.explainability_loss(ml)
        v.backward()
        torch.cuda.synchronize()
        outs.append((v.detach(), ml.grad))
    assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])
    LA.check("explain:%d:loss" % n, outs[0][0], r64[0], r32[0])
    for what, keep in (("edge", edge), ("inner", ~edge)):
        if bool(keep.any()):
            LA.check("explain:%d:dmask:%s" % (n, what), outs[0][1], r64[1], r32[1], keep=keep)


# --------------------------------------------------------------------------------------------------------------- ordinal
@pytest.mark.parametrize("name", list(LA.ORD_CASES))
def test_ordinal_head_vs_fp64(name):
    x, g, _, _ = LA.ordinal_inputs(name)
    r64, r32 = LA.ordinal_reference(name, F64), LA.ordinal_reference(name, F32)
    allowed = LA.decode_fragile(name).sum(1, keepdim=True)
    outs = {}
    for layout in LA.LAYOUTS:
        for rep in range(2):
            xl = dev(x)
            if layout == "nhwc":
                xl = xl.contiguous(memory_format=torch.channels_last)
                assert xl.stride(1) == 1
            xl.requires_grad_()
            dec, ordc = OrdinalRegressionLayer()(xl)
            (ordc * dev(g)).sum().backward()
            torch.cuda.synchronize()
            assert xl.grad.stride() == xl.stride()
            out = (ordc.detach(), dec, xl.grad.contiguous())
            if rep:
                assert all(bits_equal(a.float(), b.float()) for a, b in zip(out, outs[layout]))
            outs[layout] = out
        ordc, dec, dx = outs[layout]
        LA.check("%s:%s:ord" % (name, layout), ordc, r64[0], r32[0])
        LA.check("%s:%s:dlogits" % (name, layout), dx, r64[2], r32[2])
        assert float(dx.cpu()[(x < LA.EPS) | (x > LA.BIG)].abs().sum()) == 0.0      # logits outside the clamp get exactly no gradient
        assert dec.dtype == torch.int64 and bool(((dec.cpu() - r64[1]).abs() <= allowed).all()), "%s %s: decode" % (name, layout)
    assert all(bits_equal(a.float(), b.float()) for a, b in zip(outs["nchw"], outs["nhwc"])), "%s: the two layouts differ" % name


@pytest.mark.parametrize("name", list(LA.ORD_CASES))
def test_dorn_loss_vs_fp64(name):
    _, _, gt, target = LA.ordinal_inputs(name)
    r64, r32 = LA.dorn_reference(name, F64), LA.dorn_reference(name, F32)
    outs = []
    for _ in range(2):
        o = dev(LA.ordinal_prob32(name)).requires_grad_()
        v = LF.DORN_loss(dev(gt), o, dev(target), "kitti")
        v.backward()
        torch.cuda.synchronize()
        outs.append((v.detach(), o.grad))
    assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])
    LA.check(name + ":dorn:loss", outs[0][0], r64[0], r32[0])
    LA.check(name + ":dorn:dord", outs[0][1], r64[1], r32[1])
    assert zeros_kept(outs[0][1], r64[1]), name                  # invalid pixels, P < 1e-8, 1 - P < 1e-8


# ------------------------------------------------------------------------------------------------------------------- SID
@pytest.mark.parametrize("case", LA.SID_CASES, ids=lambda c: "K%g-%s" % c)
def test_sid_labels_at_the_bin_edges(case):
    k, ds = case
    d = LA.sid_inputs(k, ds)
    want, frag = LA.sid_reference(k, ds)
    got = UT.get_labels_sid(dev(d), ordinal_c=k, dataset=ds)
    assert got.dtype == torch.int32 and torch.equal(got, UT.get_labels_sid(dev(d), ordinal_c=k, dataset=ds))
    diff = (got.cpu() - want).abs()
    print("loss_audit sid K %g %s: %d of %d labels differ from the fp64 label, all on the %d fragile ones: %s" % (
        k, ds, int((diff > 0).sum()), d.numel(), int(frag.sum()), bool(frag[diff > 0].all())))
    assert int(diff[~frag].max()) == 0 and int(diff.max()) <= 1
    lab = torch.arange(0, int(k) + 1)
    depth = UT.get_depth_sid(dev(lab), ordinal_c=k, dataset=ds)
    LA.check("sid_depth:K%g:%s" % (k, ds), depth, LA.sid_depth_ref(lab, k, ds, F64), LA.sid_depth_ref(lab, k, ds, F32))


# -------------------------------------------------------------------------------------------------------- compute_errors
@pytest.mark.parametrize("unsupervised", (False, True))
def test_compute_errors_and_median_vs_fp64(unsupervised):
    gt, pred, _ = LA.errors_inputs(unsupervised)
    b, h, w = gt.shape
    m64, _, _ = LA.errors_ref(gt, pred, F64, True, unsupervised)
    m32, med32, _ = LA.errors_ref(gt, pred, F32, True, unsupervised)
    got = LF.compute_errors(dev(gt), dev(pred), "kitti", crop=True, unsupervised=unsupervised)
    assert got == LF.compute_errors(dev(gt), dev(pred), "kitti", crop=True, unsupervised=unsupervised)
    for i, metric in enumerate(LA.METRICS):
        LA.check("errors:median%d:%s" % (unsupervised, metric), torch.tensor(got[i], dtype=F32), m64[i], m32[i])
    # the medians, which compute_errors does not return: the raw entry point, median scaling on; bit-exactly the lower middle
    y1, y2, x1, x2 = LA.OL.garg_crop_bounds(h, w)
    scratch = torch.zeros((b, 11), dtype=F32, device=DEV)
    out8 = torch.empty(8, dtype=F32, device=DEV)
    g, p = dev(gt).contiguous(), dev(pred).contiguous()
    _lib.call("dn_compute_errors", g.data_ptr(), p.data_ptr(), b, h, w, LA.MAXD, y1, y2, x1, x2, 1, scratch.data_ptr(), out8.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    med = scratch.reshape(-1)[9 * b:11 * b].reshape(b, 2).cpu()
    print("loss_audit errors medians (gt, pred) per sample: %s" % med.tolist())
    assert bits_equal(med, med32), (med, med32)


# ---------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_reject_bad_arguments():
    """DN_ERR_BAD_ARG / DN_ERR_WORKSPACE as include/dispnet_hip.h and the DN_REQUIRE lines state them; nothing is launched"""
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=F32, device=DEV)
    p = buf.data_ptr()
    need = lib.dn_masked_loss_workspace_bytes(2, 5000)
    assert need == 2 * LA.loss_splits(5000) * 4 * 4 and lib.dn_masked_loss_workspace_bytes(0, 5000) == 0
    fwd = lambda **k: lib.dn_masked_loss_fwd(k.get("gt", p), p, k.get("G", 2), k.get("pixels", 5000), 80.0, k.get("kind", 0), 1.0, 0, p, p,
                                             k.get("ws", need), p, None)
    fused = lambda **k: lib.dn_masked_loss_fwd_fused(p, p, k.get("G", 2), k.get("pixels", 5000), 80.0, k.get("kind", 0), 1.0, 0, p, p,
                                                     k.get("ws", need), p, k.get("counter", p), None)
    big = lib.dn_masked_loss_workspace_bytes(257, 35)
    for rc, want in ((fwd(gt=None), DN_ERR_BAD_ARG), (fwd(G=0), DN_ERR_BAD_ARG), (fwd(pixels=0), DN_ERR_BAD_ARG), (fwd(kind=4), DN_ERR_BAD_ARG),
                     (fwd(kind=-1), DN_ERR_BAD_ARG), (fwd(ws=need - 1), DN_ERR_WORKSPACE),
                     (fused(counter=None), DN_ERR_BAD_ARG), (fused(kind=_lib.LOSS_BERHU), DN_ERR_BAD_ARG),
                     (fused(G=LA.FOLD_GROUPS + 1, pixels=35, ws=big), DN_ERR_BAD_ARG), (fused(ws=need - 1), DN_ERR_WORKSPACE),
                     (lib.dn_masked_loss_stats(p, p, 2, 5000, 80.0, 0, 1, p, p, need, None), DN_ERR_BAD_ARG),       # pass 1 is berHu's
                     (lib.dn_masked_loss_stats(p, p, 2, 5000, 80.0, 2, 2, p, p, need, None), DN_ERR_BAD_ARG),
                     (lib.dn_masked_loss_stats(p, p, 2, 5000, 80.0, 0, 0, p, p, need - 1, None), DN_ERR_WORKSPACE),
                     (lib.dn_masked_loss_finalize(p, 0, 0, 1.0, 0, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_masked_loss_bwd(p, p, p, None, 2, 35, 80.0, 0, 1.0, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_pyramid_down2(p, 1, 1, 8, 0, p, None), DN_ERR_BAD_ARG), (lib.dn_pyramid_down2(p, 1, 8, 8, 3, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_upsample_int_fwd(p, 1, 2, 2, 0, 0, p, None), DN_ERR_BAD_ARG), (lib.dn_upsample_int_fwd(p, 1, 2, 2, 2, 2, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_upsample_int_bwd(p, 1, 0, 2, 2, 1, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_explainability_fwd(p, 0, 1.0, 0, p, p, None), DN_ERR_BAD_ARG), (lib.dn_explainability_bwd(p, None, 8, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_compute_errors(p, p, 0, 4, 4, 80.0, 0, 4, 0, 4, 1, p, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_ordinal_fwd(p, 64, 1, 16, 1, 16, 0, p, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_ordinal_bwd(p, 64, 1, 16, p, None, 1, 16, 2, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_ordinal_loss_fwd(p, p, None, 1, 16, 2, 80.0, p, p, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_ordinal_loss_bwd(p, p, p, p, p, 1, 0, 2, 80.0, 1.0, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_ordinal_loss_finalize(None, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_sid_labels(p, 16, 80.0, 1.0, p, None), DN_ERR_BAD_ARG), (lib.dn_sid_labels(p, 0, 80.0, 80.999, p, None), DN_ERR_BAD_ARG),
                     (lib.dn_sid_depth(p, 16, 0.0, 80.999, p, None), DN_ERR_BAD_ARG)):
        assert rc == want, (rc, want, _lib.last_error())
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                      # nothing ran
