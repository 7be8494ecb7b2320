"""Host checks of tests/loss_audit.py, the fp64 audit of the supervised-loss, ordinal and error-metric kernels (no GPU needed).

  * every case fires the branch it is named for by a stated share (split count, backward elements, shares at each clamp / validity
    edge, tie counts, shares of logits and probabilities beyond 1e-8) and loses at most CAP of its elements as fragile; the cap is
    code: a tau that is too large trips it;
  * the fp32 oracle passes check() against the fp64 oracle for every case and quantity (it is `ref32`);
  * the checker rejects what it is for: fourteen fp64 mutants of the references, each at least 10 x beyond the tolerance on the case
    named.  This is the evidence that tests/test_gpu_loss_fp64.py would fail on a kernel that is wrong in that way.
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

import loss_audit as LA  # noqa: E402

F64, F32 = torch.float64, torch.float32
REJECT = 10.0               # a mutant must land at least this far beyond the tolerance


# ------------------------------------------------------------------------------------------ cases: branch shares and caps
def test_masked_cases_fire_their_branches():
    sh = {name: LA.masked_shares(name) for name in LA.MASKED_CASES}
    for name, s in sh.items():
        print("%-13s G %3d pixels %6d splits %2d | valid %.2f | pred <lo %.3f =lo %.3f =max %.3f >max %.3f | gt =0 %.3f =max %.3f >max %.3f | "
              "d==0 %.3f | r>c %.2f | ties %s empty %s" % (name, s["groups"], s["pixels"], s["splits"], s["valid"], s["pred_below"], s["pred_lo"],
                                                          s["pred_hi"], s["pred_above"], s["gt_zero"], s["gt_max"], s["gt_above"], s["zero_diff"],
                                                          s["above_c"], s["ties"][:5], s["empty"]))
    assert sh["one_split"]["splits"] == 1 and sh["one_split"]["groups"] == 3
    assert sh["two_splits"]["pixels"] == 2049 and sh["two_splits"]["splits"] == 2
    assert sh["split_cap"]["pixels"] > 63 * LA.LOSS_SPLIT_PIXELS and sh["split_cap"]["splits"] == LA.LOSS_SPLIT_MAX and sh["split_cap"]["groups"] == 1
    assert sh["bwd_grid_cap"]["elems"] > LA.BWD_GRID_ELEMS
    assert sh["groups_256"]["groups"] == LA.FOLD_GROUPS and sh["groups_257"]["groups"] == LA.FOLD_GROUPS + 1
    for name in ("one_split", "two_splits", "split_cap", "groups_256", "groups_257"):      # the generic inputs reach both clamp sides
        s = sh[name]
        assert s["pred_below"] >= 0.05 and s["pred_above"] >= 0.05 and s["gt_zero"] >= 0.03 and s["gt_max"] >= 0.03 and s["gt_above"] >= 0.03, name
        assert not s["empty"], name
    s = sh["clamp_edges"]
    for key in ("pred_below", "pred_lo", "pred_hi", "pred_above", "gt_zero", "gt_max"):
        assert s[key] >= 0.08, key
    assert sh["l1_zero_diff"]["zero_diff"] >= 0.15
    assert sh["empty_group"]["empty"] == [1]
    s = sh["berhu_ties"]
    assert tuple(s["ties"]) == LA.TIE_COUNTS and s["max_r"] == [LA.TIE_R] * 3 and 0.2 <= s["above_c"] <= 0.8
    s = sh["berhu_flat"]
    assert s["max_r"] == [0.0, 0.0] and s["valid"] >= 0.5 and s["zero_diff"] == s["valid"]


def test_multiscale_upsample_explain_cases():
    gt, preds = LA.multiscale_inputs()
    assert [tuple(p.shape[2:]) for p in preds] == [(24, 40), (12, 20), (6, 10), (3, 5)]
    for pool in ("max", "avg", "bilinear"):                 # the pyramids stay on a dyadic grid: exact in fp32
        for a, b in zip(LA.OL._gt_pyramid(gt, pool), LA.OL._gt_pyramid(gt.double(), pool)):
            assert torch.equal(a.double(), b)
    assert LA.UPSAMPLE["sizes"][0] == (1, 1) and set(LA.UPSAMPLE["scales"]) == {1, 2, 4, 8}
    assert LA.EXPLAIN_SIZES[0] == 1 and LA.EXPLAIN_SIZES[1] == 257 and LA.EXPLAIN_SIZES[2] > LA.REDUCE1D_ELEMS
    for n in LA.EXPLAIN_SIZES[1:]:
        m, edge = LA.explain_inputs(n)
        x = m.double()
        f = lambda c: float(c.double().mean())
        print("explain %6d: edge %.3f | == 1 %.3f | log clamps %.3f | (1-x)x < 1e-12 %.3f" % (n, f(edge), f(m == 1), f(x < 3.7e-44), f((1 - x) * x < 1e-12)))
        assert f(m == 1) >= 0.01 and f(x < 3.7e-44) >= 0.02 and f((1 - x) * x < 1e-12) >= 0.05
        assert bool(((m > 0.04) | edge).all())


@pytest.mark.parametrize("name", sorted(LA.ORD_CASES))
def test_ordinal_cases_fire_their_branches(name):
    s = LA.dorn_shares(name)
    frag = LA.decode_fragile(name)                           # asserts the cap itself
    print("%s: logits < 0 %.3f, in [0, 1e-8) %.3f, > 1e8 %.3f | P < 1e-8 %.3f, 1 - P == 0 %.3f, 1 - P < 1e-8 %.3f | gt invalid %.2f | "
          "targets %s | decode fragile %.4f" % (name, s["neg"], s["tiny"], s["big"], s["p_small"], s["q_zero"], s["q_small"], s["invalid"],
                                                s["targets"], float(frag.double().mean())))
    k = s["K"]
    assert s["neg"] >= 0.08 and s["tiny"] >= 0.03 and s["big"] >= 0.03
    assert s["p_small"] >= 0.03 and s["q_zero"] >= 0.03
    assert 0.15 <= s["invalid"] <= 0.35
    assert s["targets"] == sorted({0, k // 2, k, k + 3})
    assert float(frag.double().mean()) <= LA.CAP


def test_sid_and_errors_cases_within_cap():
    for k, ds in LA.SID_CASES:
        lab, frag = LA.sid_reference(k, ds)                  # asserts the cap itself
        d = LA.sid_inputs(k, ds)
        v32 = LA.sid_value(d, k, ds, F32).trunc().to(torch.int32)
        print("sid K %g %s: %d depths, labels %d .. %d, fragile %.4f, fp32 labels differ on %d (all fragile: %s)" % (
            k, ds, d.numel(), int(lab.min()), int(lab.max()), float(frag.double().mean()), int((v32 != lab).sum()), bool(frag[v32 != lab].all())))
        assert int(lab.min()) == 0 and int(lab.max()) >= k - 1
        assert int(frag.sum()) >= 2 * k                       # the neighbours of the edges are in
        assert bool(frag[v32 != lab].all()) and int((v32 - lab).abs().max()) <= 1      # the reference alone: within +-1, on fragile labels only
        assert float(frag.double().mean()) <= LA.CAP
    for uns in (False, True):
        c = LA.errors_counts(uns)
        print("errors_median (median scaling %d): valid counts %s, removed as fragile %d, clamped low %.2f high %.2f" % (
            uns, c["counts"], c["removed"], c["clamped_lo"], c["clamped_hi"]))
        assert c["counts"][0] % 2 == 0 and c["counts"][1] % 2 == 1 and c["counts"][2] == 1
        assert c["clamped_lo"] >= 0.1 and c["clamped_hi"] >= 0.3
        gt, pred, _ = LA.errors_inputs(uns)
        _, _, thrs = LA.errors_ref(gt, pred, F64, True, uns)
        for _, thr in thrs:
            for t in LA.THR:
                assert not bool(((thr - t).abs() < LA.TAU_THR * t).any())


def test_fragile_cap_is_enforced():
    """a tau that flags far more than CAP trips the assertion inside the functions (the cap is code, not prose)"""
    for attr, big, clear, call in (("TAU_SID", 0.05, LA.sid_reference, lambda: LA.sid_reference(*LA.SID_CASES[0])),
                                   ("TAU_P", 0.45, LA.decode_fragile, lambda: LA.decode_fragile("ord_K8")),
                                   ("TAU_THR", 0.05, LA.errors_inputs, lambda: LA.errors_inputs(False))):
        old = getattr(LA, attr)
        clear.cache_clear()
        try:
            setattr(LA, attr, big)
            with pytest.raises(AssertionError, match="fragile"):
                call()
        finally:
            setattr(LA, attr, old)
            clear.cache_clear()


# ------------------------------------------------------------------------------------- the fp32 oracle passes trivially
def _ck(tag, r32, r64):
    return LA.check(tag, r32, r64, r32, verbose=False)


def test_fp32_oracle_passes():
    for name in LA.MASKED_CASES:
        for kind in LA.KINDS:
            if name in ("berhu_ties", "berhu_flat") and kind != "berhu":
                continue
            (l64, g64), (l32, g32) = LA.per_sample_reference(name, kind, F64), LA.per_sample_reference(name, kind, F32)
            if name == "empty_group":
                assert bool(torch.isnan(l64)) and bool(torch.isnan(l32)) and float(g64[1].abs().max()) == 0.0
            elif name != "bwd_grid_cap":
                _ck("%s:%s:loss" % (name, kind), l32, l64)
            if name == "berhu_flat":
                assert float(l64) == 0.0 and float(g64.abs().max()) == 0.0 and float(g32.abs().max()) == 0.0
            else:
                _ck("%s:%s:dpred" % (name, kind), g32, g64)
    for fn, pool, kind in LA.MULTISCALE_RUNS:
        r64, r32 = LA.multiscale_reference(fn, pool, kind, F64), LA.multiscale_reference(fn, pool, kind, F32)
        _ck("%s:%s:loss" % (fn, pool), r32[0], r64[0])
        for i in range(4):
            _ck("%s:%s:dpred%d" % (fn, pool, i), r32[1][i], r64[1][i])
    for size in LA.UPSAMPLE["sizes"]:
        for scale in LA.UPSAMPLE["scales"]:
            for mode in LA.UPSAMPLE["modes"]:
                r64, r32 = LA.upsample_reference(size, scale, mode, F64), LA.upsample_reference(size, scale, mode, F32)
                _ck("upsample:out", r32[0], r64[0])
                _ck("upsample:dx", r32[1], r64[1])
    for n in LA.EXPLAIN_SIZES:
        r64, r32 = LA.explain_reference(n, F64), LA.explain_reference(n, F32)
        _, edge = LA.explain_inputs(n)
        _ck("explain:%d:loss" % n, r32[0], r64[0])
        for keep in (edge, ~edge):
            if bool(keep.any()):
                LA.check("explain:%d:dmask" % n, r32[1], r64[1], r32[1], keep=keep, verbose=False)
    for name in LA.ORD_CASES:
        r64, r32 = LA.ordinal_reference(name, F64), LA.ordinal_reference(name, F32)
        _ck(name + ":ord", r32[0], r64[0])
        _ck(name + ":dlogits", r32[2], r64[2])
        assert bool(((r32[1] - r64[1]).abs() <= LA.decode_fragile(name).sum(1, keepdim=True)).all())
        d64, d32 = LA.dorn_reference(name, F64), LA.dorn_reference(name, F32)
        _ck(name + ":dorn:loss", d32[0], d64[0])
        _ck(name + ":dorn:dord", d32[1], d64[1])
    for k, ds in LA.SID_CASES:
        lab = torch.arange(0, int(k) + 1)
        _ck("sid_depth", LA.sid_depth_ref(lab, k, ds, F32), LA.sid_depth_ref(lab, k, ds, F64))
    for uns in (False, True):
        gt, pred, _ = LA.errors_inputs(uns)
        m64, med64, _ = LA.errors_ref(gt, pred, F64, True, uns)
        m32, med32, _ = LA.errors_ref(gt, pred, F32, True, uns)
        assert torch.equal(med32.double(), med64)               # a selection: the same fp32 numbers in either precision
        for i, metric in enumerate(LA.METRICS):
            _ck("errors:%s" % metric, m32[i], m64[i])


# ------------------------------------------------------------------------------------------------------------ the mutants
def _excess(tag, got, r64, r32, keep=None):
    r = LA.compare(tag, got, r64, r32, keep)
    print("mutant %-58s worst / tol %.3g" % (tag, r.excess))
    return r.excess


def _masked_mutant(name, kind, mutant, what):
    r64, r32, m = (LA.per_sample_reference(name, kind, F64), LA.per_sample_reference(name, kind, F32),
                   LA.per_sample_reference(name, kind, F64, mutant))
    i = 0 if what == "loss" else 1
    return _excess("%s on %s:%s:%s" % (mutant, name, kind, what), m[i], r64[i], r32[i])


def test_masked_mutants_are_rejected():
    assert _masked_mutant("clamp_edges", "l1", "valid_le_max", "loss") >= REJECT
    assert _masked_mutant("clamp_edges", "l1", "valid_le_max", "dpred") >= REJECT
    for kind in LA.KINDS:
        assert _masked_mutant("clamp_edges", kind, "clamp_passes", "dpred") >= REJECT
    assert _masked_mutant("berhu_ties", "berhu", "berhu_tie_whole", "dpred") >= REJECT
    assert _masked_mutant("berhu_ties", "berhu", "berhu_no_c_path", "dpred") >= REJECT
    assert _masked_mutant("one_split", "scale_inv", "si_factor", "loss") >= REJECT
    assert _masked_mutant("one_split", "scale_inv", "si_factor", "dpred") >= REJECT
    for kind in LA.KINDS:
        assert _masked_mutant("one_split", kind, "mean_all", "loss") >= REJECT
        assert _masked_mutant("one_split", kind, "whole_batch", "loss") >= REJECT
        assert _masked_mutant("one_split", kind, "whole_batch", "dpred") >= REJECT


def test_multiscale_and_upsample_mutants_are_rejected():
    for fn, pool, kind in LA.MULTISCALE_RUNS:
        r64, r32, m = (LA.multiscale_reference(fn, pool, kind, F64), LA.multiscale_reference(fn, pool, kind, F32),
                       LA.multiscale_reference(fn, pool, kind, F64, "weights_swapped"))
        assert _excess("weights_swapped on %s:%s:loss" % (fn, pool), m[0], r64[0], r32[0]) >= REJECT
        assert _excess("weights_swapped on %s:%s:dpred3" % (fn, pool), m[1][3], r64[1][3], r32[1][3]) >= REJECT
    args = ("Multiscale_FULL_L1_loss", "bilinear", "l1")
    r64, r32, m = LA.multiscale_reference(*args, F64), LA.multiscale_reference(*args, F32), LA.multiscale_reference(*args, F64, "align_corners")
    assert _excess("align_corners on Multiscale_FULL_L1_loss:loss", m[0], r64[0], r32[0]) >= REJECT
    for size in LA.UPSAMPLE["sizes"][1:]:
        for scale in (2, 4, 8):
            a = (size, scale, "bilinear")
            r64, r32, m = LA.upsample_reference(*a, F64), LA.upsample_reference(*a, F32), LA.upsample_reference(*a, F64, "align_corners")
            assert _excess("align_corners on upsample %s x%d:out" % a[:2], m[0], r64[0], r32[0]) >= REJECT
            assert _excess("align_corners on upsample %s x%d:dx" % a[:2], m[1], r64[1], r32[1]) >= REJECT


@pytest.mark.parametrize("name", sorted(LA.ORD_CASES))
def test_ordinal_mutants_are_rejected(name):
    r64, r32 = LA.ordinal_reference(name, F64), LA.ordinal_reference(name, F32)
    for mutant in ("ord_clamp_passes", "strides_swapped"):
        m = LA.ordinal_reference(name, F64, mutant)
        assert _excess("%s on %s:dlogits" % (mutant, name), m[2], r64[2], r32[2]) >= REJECT
    d64, d32 = LA.dorn_reference(name, F64), LA.dorn_reference(name, F32)
    for mutant in ("k_le_t", "one_minus_p_unclamped"):
        m = LA.dorn_reference(name, F64, mutant)
        assert _excess("%s on %s:dorn:loss" % (mutant, name), m[0], d64[0], d32[0]) >= REJECT
    m = LA.dorn_reference(name, F64, "k_le_t")
    assert _excess("k_le_t on %s:dorn:dord" % name, m[1], d64[1], d32[1]) >= REJECT


def test_median_mutant_is_rejected():
    gt, pred, _ = LA.errors_inputs(True)
    m64, med64, _ = LA.errors_ref(gt, pred, F64, True, True)
    m32, _, _ = LA.errors_ref(gt, pred, F32, True, True)
    mm, medm, _ = LA.errors_ref(gt, pred, F64, True, True, "upper_median")
    assert not torch.equal(medm[0], med64[0]) and torch.equal(medm[1:], med64[1:])       # only the even count has two middles
    for i in range(5):                                          # the metrics that vary with the scale (a1-a3 are counts and may stay)
        assert _excess("upper_median on errors:%s" % LA.METRICS[i], mm[i], m64[i], m32[i]) >= REJECT


def test_every_listed_mutant_has_a_test():
    src = open(os.path.abspath(__file__)).read()
    for mutant in LA.MUTANTS:
        assert src.count('"%s"' % mutant) >= 1, mutant
