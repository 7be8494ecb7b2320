"""The fp64 audit of monodepth2's multi-scale objective checks itself on the CPU: its restatement (tests/mono2_audit.py) meets the
golden recorded from the reference's own layers, its cases keep the fragile pixels below the cap at every scale and exercise what
they are named for, every mutant of the objective lands beyond the tolerance, and train.py knows --min-reprojection."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mono2_audit as MA  # noqa: E402

F64, F32 = torch.float64, torch.float32
MODES = [(ac, am) for ac in MA.ALIGNS for am in MA.AUTOMASKS]


@pytest.mark.parametrize("align,automask", MODES)
def test_restatement_meets_the_reference_golden(golden, align, automask):
    g = golden("mono2_loss")
    r32 = MA.reference("ms_select", align, automask, F32)
    tag = "ms_select:ac%d:am%d:" % (align, automask)
    want_parts, want_loss = torch.as_tensor(g[tag + "parts"]), float(g[tag + "loss"])
    # two fp32 evaluations of one formula chain (the reference's SSIM / Project3D modules against the restatement's functions)
    assert float((r32["parts"].double() - want_parts).abs().max()) <= 1e-6 * float(want_parts.abs().max())
    assert abs(float(r32["loss"]) - want_loss) <= 1e-6 * abs(want_loss)
    r64 = MA.reference("ms_select", align, automask, F64)
    assert abs(float(r64["loss"]) - want_loss) <= 1e-5 * abs(want_loss)


@pytest.mark.parametrize("name", MA.FULL_CASES)
def test_cases_keep_the_cap_at_every_scale(name):
    for align, automask in MODES:
        fr = MA.fragile(name, align, automask)                      # asserts the cap per scale
        assert len(fr) == MA.S_MAX
        w = MA.weights(name, align, automask)
        assert tuple(w.shape) == (MA.S_MAX,) + tuple(fr[0].shape)
        assert all(float(w[s][fr[s]].abs().max()) == 0.0 for s in range(MA.S_MAX) if bool(fr[s].any()))
    c = MA.CASES[name]
    assert c["H"] % 8 == 0 and c["W"] % 8 == 0


def test_selection_case_lets_every_channel_win_at_every_scale():
    for align in MA.ALIGNS:
        for shares in MA.win_shares("ms_select", align):
            assert len(shares) == 4 and min(shares) >= 0.15, shares


def test_value_case_weights_are_zero_and_its_maps_end_in_one_pixel():
    i = MA.inputs("ms_one")
    assert tuple(i["disps"][3].shape) == (1, 1, 1, 1) and tuple(MA.inputs("ms_small")["disps"][3].shape) == (2, 1, 1, 2)
    assert float(MA.weights("ms_one", False, True).abs().max()) == 0.0
    r = MA.reference("ms_one", False, True, F64)
    assert torch.isfinite(r["loss"]) and torch.isfinite(r["parts"]).all()
    assert float(r["parts"][3, 1]) == 0.0 and float(r["parts"][2, 1]) > 0.0         # a one-pixel map has no neighbour pair
    assert all(float(g.abs().max()) > 0 for g in r["ddisp"][:3])                     # the smoothness gradient alone


def _mutant_factor(name, align, automask, mutant):
    """the worst of |mutant - ref64| / tolerance over the loss and the two columns of the per-scale parts"""
    r64, r32 = MA.reference(name, align, automask, F64), MA.reference(name, align, automask, F32)
    m = MA.reference(name, align, automask, F64, mutant=mutant)
    worst = 0.0
    for q, sl in (("loss", None), ("reprojection", 0), ("smoothness", 1)):
        pick = (lambda r: r["loss"]) if sl is None else (lambda r: r["parts"][:, sl])
        worst = max(worst, MA.compare(mutant + ":" + q, pick(m), pick(r64), pick(r32)).excess)
    return worst


@pytest.mark.parametrize("mutant", MA.MUTANTS)
def test_every_mutant_lands_beyond_the_tolerance(mutant):
    factors = []
    for align, automask in MODES:
        if mutant == "coarse_identity" and not automask:
            continue                                                 # no identity terms to take at the coarse resolution
        factors.append(_mutant_factor("ms_select", align, automask, mutant))
    print("mutant %-16s x tolerance: %s" % (mutant, ", ".join("%.3g" % f for f in factors)))
    assert min(factors) > 1.0, (mutant, factors)


def test_restatement_passes_its_own_check():
    r64, r32 = MA.reference("ms_select", False, True, F64), MA.reference("ms_select", False, True, F32)
    MA.check("self:loss", r32["loss"], r64["loss"], r32["loss"])
    for s in range(MA.S_MAX):
        MA.check("self:ddisp%d" % s, r32["ddisp"][s], r64["ddisp"][s], r32["ddisp"][s])


# ---------------------------------------------------------------------------------------------------------------- train.py
def test_train_help_lists_min_reprojection():
    import train
    text = train.build_parser().format_help()
    for flag in ("--min-reprojection", "--min-depth", "--max-depth", "--no-automask"):
        assert flag in text, flag


def test_min_reprojection_needs_unsupervised_monodepth2():
    import train
    for argv in (["DIR", "--min-reprojection"], ["DIR", "--min-reprojection", "--unsupervised"], ["DIR", "--min-reprojection", "--monodepth2"]):
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert "--unsupervised --monodepth2" in str(e.value)


def test_homogeneous_intrinsics():
    import train
    k = torch.tensor([[[100.0, 0, 47.5], [0, 101.0, 32.0], [0, 0, 1]]]).repeat(2, 1, 1)
    k4 = train._homogeneous(k)
    assert tuple(k4.shape) == (2, 4, 4) and torch.equal(k4[:, :3, :3], k) and float(k4[0, 3, 3]) == 1.0
    assert float(k4[:, 3, :3].abs().max()) == 0.0 and float(k4[:, :3, 3].abs().max()) == 0.0
    assert torch.allclose(train._homogeneous(torch.inverse(k)), torch.inverse(k4))
