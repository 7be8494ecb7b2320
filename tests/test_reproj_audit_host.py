"""Host checks of tests/reproj_audit.py, the fp64 audit of the monodepth2 self-supervision kernels (no GPU needed).

  * the restatement of the reference's layers.py (pose matrices, BackprojectDepth, Project3D, the minimum-reprojection composition)
    and of its PoseCNN equals the golden recorded from the reference itself (tests/golden/make_reproj_goldens.py);
  * every case stays within the fragile-pixel cap, the selection case gives every channel its share, and each case fires what it is
    named for (out-of-image share, points behind the camera, more than one tile in each direction);
  * the fp32 restatement passes check() against the fp64 one (it is `ref32`);
  * the checker rejects what it is for: six fp64 mutants, each at least 10 x beyond the tolerance on the case named.  This is the
    evidence that tests/test_gpu_reproj.py would fail on a kernel that is wrong in that way;
  * networks.PoseCNN constructs with the reference's state_dict keys.
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

import reproj_audit as RA  # noqa: E402

F64, F32 = torch.float64, torch.float32
REJECT = 10.0               # a mutant must land at least this far beyond the tolerance
MODES = [(ac, am) for ac in RA.ALIGNS for am in RA.AUTOMASKS]


def _close(got, want, rtol=2e-5, atol_rel=2e-6):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape
    return bool(((got - want).abs() <= atol_rel * float(want.abs().max()) + rtol * want.abs()).all())


# ---------------------------------------------------------------------------------------------- the restatement is the reference
def test_restatement_equals_the_golden(golden):
    g = golden("reproj")
    aa, tr = RA.pose_vectors()
    assert _close(RA.rot_from_axisangle(aa), g["pose:rot"]) and _close(RA.get_translation_matrix(tr), g["pose:trans"])
    for inv in (False, True):
        m, daa, dt = RA.pose_reference(inv, F32)
        assert _close(m, g["pose:M:inv%d" % inv]) and _close(daa, g["pose:daa:inv%d" % inv]) and _close(dt, g["pose:dt:inv%d" % inv])
    for size in RA.GEOM_SIZES:
        r, tag = RA.geom_reference(size, F32), "geom:%dx%d:" % size
        for q in ("points", "grid", "ddepth", "dT"):
            assert _close(r[q], g[tag + q], rtol=1e-4, atol_rel=1e-5), (size, q)
    for ac, am in MODES:
        r = RA.reference("select_ragged", ac, am, F32)
        # (SSIM in fp32 loses ~1e-5 of a term to cancellation in whichever order it is evaluated; the orders are the same here)
        assert _close(r["m"], g["loss:select_ragged:ac%d:am%d:m" % (ac, am)], rtol=1e-4, atol_rel=1e-4)
        assert abs(float(r["loss"]) - float(g["loss:select_ragged:ac%d:am%d:loss" % (ac, am)])) <= 1e-5 * float(r["loss"])
    a, t, grads = RA.pose_cnn_reference(F32)
    assert _close(a, g["posecnn:axisangle"], rtol=1e-4, atol_rel=1e-5) and _close(t, g["posecnn:translation"], rtol=1e-4, atol_rel=1e-5)
    for k in RA.POSE_CNN_KEYS:
        want = g["posecnn:grad:%s:samples" % k]
        got = grads[k].double().reshape(-1).numpy()[::53]
        assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max() + 1e-12, k
    assert list(g["posecnn:keys"]) == sorted(RA.POSE_CNN_KEYS, key=list(g["posecnn:keys"]).index)


def test_pose_cnn_constructs_with_the_reference_keys(golden):
    import supervised_dispnet_amd.networks as networks
    net = networks.PoseCNN(2)
    assert net.num_input_frames == 2
    assert list(net.state_dict().keys()) == list(golden("reproj")["posecnn:keys"])
    sd = RA.pose_cnn_state()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert tuple(networks.PoseCNN(3).pose_conv.weight.shape) == (12, 256, 1, 1)
    for name in ("PoseDecoder",):
        with pytest.raises(NotImplementedError):
            getattr(networks, name)()


# ------------------------------------------------------------------------------------------ cases: caps, shares, what they fire
@pytest.mark.parametrize("name", RA.LOSS_CASES)
def test_fragile_share_within_cap(name):
    for ac, am in MODES:
        share = float(RA.fragile(name, ac, am).double().mean())          # asserts the cap itself
        print("%s align %d automask %d: %.2f %% fragile" % (name, ac, am, 100 * share))
        assert share <= RA.CAP
    assert RA.CAP == 0.12


def test_fragile_cap_is_enforced():
    tau = RA.TAU_PX
    RA.fragile.cache_clear()
    try:
        RA.TAU_PX = 0.1
        with pytest.raises(AssertionError, match="fragile"):
            RA.fragile("seams", False, True)
    finally:
        RA.TAU_PX = tau
        RA.fragile.cache_clear()


def test_selection_case_gives_every_channel_its_share():
    for ac in RA.ALIGNS:
        shares = RA.win_shares("select_ragged", ac)
        print("select_ragged align %d: win shares %s" % (ac, ["%.3f" % s for s in shares]))
        assert len(shares) == 4 and min(shares) >= RA.MIN_WIN


def test_cases_fire_what_they_are_named_for():
    tiles = lambda c: (-(-c["H"] // RA.TILE_H), -(-c["W"] // RA.TILE_W))
    c = RA.CASES["select_ragged"]
    assert c["H"] % RA.TILE_H and c["W"] % RA.TILE_W and min(tiles(c)) >= 2 and c["F"] == 2 and c["B"] == 3
    assert min(tiles(RA.CASES["seams"])) >= 3 and RA.CASES["seams"]["F"] == 2           # interior tiles: seams on all four sides
    assert RA.CASES["large_motion"]["F"] == 3
    for ac in RA.ALIGNS:
        out, behind = RA.motion_shares("large_motion", ac)
        print("large_motion align %d: %.1f %% of the coordinates outside the image, %.1f %% of the points behind the camera" % (ac, 100 * out, 100 * behind))
        assert out >= 0.10 and behind > 0.02
    for name in ("min_2x2", "min_3x3"):
        assert RA.CASES[name]["F"] == 1 and RA.CASES[name]["B"] == 1
    i = RA.inputs("twins")
    assert torch.equal(i["refs"][0], i["refs"][1]) and torch.equal(i["T"][0], i["T"][1])
    aa, _ = RA.pose_vectors()
    assert float(aa.norm(dim=2).max()) > 2.9 and RA.POSE_CASE["B"] == 5


# --------------------------------------------------------------------------------------- the fp32 restatement passes trivially
def test_fp32_restatement_passes():
    for name in RA.LOSS_CASES:
        for ac, am in MODES:
            r64, r32 = RA.reference(name, ac, am, F64), RA.reference(name, ac, am, F32)
            for q in ("m", "loss", "ddisp"):
                RA.check("%s:%s" % (name, q), r32[q], r64[q], r32[q], verbose=False)
            for f in range(len(r64["dT"])):
                RA.check("%s:dT%d" % (name, f), r32["dT"][f], r64["dT"][f], r32["dT"][f], verbose=False)
            off_tie = ~r64["near_tie"]
            assert torch.equal(r32["sel"][off_tie], r64["sel"][off_tie]), (name, ac, am)


# ------------------------------------------------------------------------------------------------------------- the mutants
def _mutant(name, align, automask, ties=True, T=None, **switches):
    """the fp64 composition with `switches` flipped, under the upstream map of the TRUE mode: dict(m, loss, ddisp, dT)"""
    i = RA.inputs(name)
    d = lambda t: t.double()
    disp = RA._leaf(i["disp"], F64)
    Ts = [RA._leaf(t, F64) for t in (T if T is not None else i["T"])]
    ev = RA.evaluate(d(i["tgt"]), [d(r) for r in i["refs"]], disp, d(i["K"]), d(i["inv_K"]), Ts, switches.pop("eval_align", align), automask, **switches)
    (ev["m"] * RA.upstream(name, align, automask, ties).double()).sum().backward()
    zero = lambda t, like: t if t is not None else torch.zeros_like(like)
    return dict(m=ev["m"].detach(), loss=ev["loss"].detach(), ddisp=zero(disp.grad, disp), dT=[zero(t.grad, t) for t in Ts])


def _excess(name, align, automask, got, ties=True):
    r64, r32 = RA.reference(name, align, automask, F64, ties), RA.reference(name, align, automask, F32, ties)
    ex = {q: RA.compare(q, got[q], r64[q], r32[q]).excess for q in ("m", "loss", "ddisp")}
    for f in range(len(r64["dT"])):
        ex["dT%d" % f] = RA.compare("dT", got["dT"][f], r64["dT"][f], r32["dT"][f]).excess
    return ex


def _report(n, what, ex):
    print("mutant %d %-66s %s" % (n, what, "  ".join("%s %.3g x" % kv for kv in sorted(ex.items()))))


def test_unmutated_composition_passes():
    for name in RA.LOSS_CASES:
        for ac, am in MODES:
            ex = _excess(name, ac, am, _mutant(name, ac, am))
            assert max(ex.values()) <= 1.0, (name, ac, am, ex)


def test_mutant_1_wrong_tie_order():
    """a tie that goes to the HIGHEST channel: invisible in m, but on twin frames the gradient lands on the other frame's T"""
    for am in RA.AUTOMASKS:
        ex = _excess("twins", False, am, _mutant("twins", False, am, ties=False, tie_last=True), ties=False)
        _report(1, "ties go to the highest channel (twins, automask %d)" % am, ex)
        assert ex["dT0"] >= REJECT and ex["dT1"] >= REJECT and ex["m"] <= 1.0


def test_mutant_2_align_corners_swapped():
    for name in ("select_ragged", "seams"):
        for ac, am in MODES:
            ex = _excess(name, ac, am, _mutant(name, ac, am, eval_align=not ac))
            _report(2, "align_corners %d computed as %d (%s, automask %d)" % (ac, not ac, name, am), ex)
            assert min(ex[q] for q in ("m", "loss", "ddisp")) >= REJECT


def test_mutant_3_zeros_for_border():
    """(automask off: on large_motion the identity terms win every pixel otherwise, and no reprojection term reaches m)"""
    for ac in RA.ALIGNS:
        ex = _excess("large_motion", ac, False, _mutant("large_motion", ac, False, padding="zeros"))
        _report(3, "zeros padding for border (large_motion, align %d)" % ac, ex)
        assert min(ex[q] for q in ("m", "loss", "ddisp")) >= REJECT


def test_mutant_4_clamp_on_the_projected_depth():
    for ac in RA.ALIGNS:
        ex = _excess("large_motion", ac, False, _mutant("large_motion", ac, False, clamp_z=True))
        _report(4, "c[2] clamped at 1e-3 as inverse_warp does (large_motion, align %d)" % ac, ex)
        assert min(ex[q] for q in ("m", "loss", "ddisp")) >= REJECT


def test_mutant_5_x_divided_by_w():
    for name in ("select_ragged", "seams"):
        for ac, am in MODES:
            ex = _excess(name, ac, am, _mutant(name, ac, am, div_w=True))
            _report(5, "x / W for x / (W - 1) (%s, align %d, automask %d)" % (name, ac, am), ex)
            assert min(ex[q] for q in ("m", "loss", "ddisp")) >= REJECT


def test_mutant_6_inverted_pose_composed_in_the_wrong_order():
    aa, tr = RA.pose_vectors()
    r64, r32 = RA.pose_reference(True, F64), RA.pose_reference(True, F32)
    got = RA.pose_reference(True, F64, True)
    ex = {q: RA.compare(q, got[k], r64[k], r32[k]).excess for k, q in enumerate(("M", "daxisangle", "dtranslation"))}
    _report(6, "T R where R^T T(-t) is asked for (pose matrices, 3 rad)", ex)
    assert min(ex.values()) >= REJECT
    # and through the loss: the selection case has an inverted frame
    i = RA.inputs("select_ragged")
    assert i["invert"][1]
    T = [RA.transformation_from_parameters(i["axisangle"][:, f].double(), i["translation"][:, f].double(), i["invert"][f], mutant_order=True).float()
         for f in range(2)]
    ex = _excess("select_ragged", False, False, _mutant("select_ragged", False, False, T=T))
    _report(6, "the same through the loss (select_ragged)", ex)
    assert min(ex[q] for q in ("m", "loss", "ddisp")) >= REJECT
