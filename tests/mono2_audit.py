"""fp64 audit of monodepth2's multi-scale objective (csrc/dn_mono2.hip, loss_functions.monodepth2_loss): the cases, the torch
restatement and the fragile-pixel rule per scale (a plain module, importable without a GPU).  The layers, the tolerance rule
(check / compare, MARGIN = 16 x the fp32 restatement's own error against fp64 + 4 u max|ref64|), the fragile-pixel thresholds and
the 12 % cap are those of reproj_audit.py, unchanged; the smoothness part is compared by the same check(), as geom_audit does for
get_smooth_loss.

The yardstick, evaluated by torch on the CPU in fp64 and in fp32, per scale s of S:
    up_s    = F.interpolate(disps[s], (H, W), mode="bilinear", align_corners=False)
    m_s     = reproj_audit.evaluate(tgt, refs, up_s, ...)["m"]           (depth = disp_to_depth(up_s), identity terms at full resolution)
    norm_s  = disps[s] / (disps[s].mean((2, 3), keepdim=True) + 1e-7)
    loss    = (1 / S) * sum_s [ (m_s * weight_s).mean() + SMOOTHNESS / 2^s * get_smooth_loss(norm_s, area-interpolated tgt) ]
weight_s = 1 for the values; for the gradients it is the case's upstream map g_s with ZERO on the fragile pixels of scale s (found
from the fp64 evaluation of that scale), so that neither side's gradient sees them -- the rule of reproj_audit.py, applied per
scale; fragile() asserts the cap for every scale.  A direction in which a map has no neighbour pair (the 1 x 2 and 1 x 1 maps of
ms_small and ms_one) contributes 0 to its smoothness.

SMOOTHNESS = 0.05, fifty times monodepth2's 1e-3: at 1e-3 the smoothness gradient is some 1e-3 of the reprojection gradient in
every ddisp_s and a wrong smoothness backward would hide below the tolerance of the sum.

The cases: each is the recipe of a reproj_audit.CASES entry at another size, registered under its own name so that
reproj_audit.inputs() builds it; the disparity of scale s is the recipe's formula on the (H >> s) x (W >> s) grid with the pattern
tag "reproj:<case>:disp<s>".  ms_one's coarse maps are too small for the cap (14.1 % at scale 2 without align_corners): its values
and its smoothness gradient (weight_s = 0) are compared, nothing else.

Measured on an MI355X (tests/test_gpu_mono2.py prints every figure), 5 cases x align_corners x automask: no quantity needs more than
0.12 of the tolerance (the smoothness gradient ddisp0 of ms_one; dT0 of ms_select 0.11, at 1.8 x the fp32 restatement's own error).
"""
import functools

import torch
import torch.nn.functional as F

import reproj_audit as RA
from oracle import detgen
from reproj_audit import CAP, FLOOR, MARGIN, check, compare  # noqa: F401

S_MAX = 4
SMOOTHNESS = 0.05

CASES = {
    # recipe of min_2x2: the coarsest map is 1 x 2, both bilinear neighbours clamp
    "ms_small": dict(B=2, H=8, W=16, F=1, shift=((0.7, 0.3),), trans=0.1, rot=0.05, pert=0.6),
    # recipe of select_ragged: 40 = 32 + 8 against the tile; every one of the four channels wins its share at every scale
    "ms_select": dict(RA.CASES["select_ragged"], B=2, H=24, W=40),
    # recipe of seams
    "ms_seams": dict(RA.CASES["seams"], B=1, H=40, W=136),
    # recipe of large_motion
    "ms_motion": dict(RA.CASES["large_motion"], B=2, H=24, W=40),
    # recipe of min_2x2: the coarsest map is one pixel
    "ms_one": dict(RA.CASES["min_2x2"], B=1, H=8, W=8),
}
RA.CASES.update(CASES)
FULL_CASES = ("ms_small", "ms_select", "ms_seams", "ms_motion")      # everything is compared
VALUE_CASES = ("ms_one",)                                            # values and the smoothness gradient only
ALIGNS, AUTOMASKS = RA.ALIGNS, RA.AUTOMASKS


@functools.lru_cache(maxsize=None)
def inputs(name):
    """reproj_audit.inputs(name) plus `disps` (S_MAX maps) and `g` (S_MAX upstream maps, not yet masked)"""
    i = dict(RA.inputs(name))
    c = CASES[name]
    b, h, w = c["B"], c["H"], c["W"]
    tag = "reproj:" + name
    disps = []
    for s in range(S_MAX):
        d = 0.02 + 0.06 * (RA.pattern(b, h >> s, w >> s, tag + ":disp%d" % s)[:, :1] - 0.1) / 0.8
        if c.get("select"):
            d = 0.024 + 0.15 * (d - 0.05)
        disps.append(d.float())
    i["disps"] = disps
    i["g"] = [detgen.uniform((b, 1, h, w), tag + ":g%d" % s, 0.2, 1.0) for s in range(S_MAX)]
    return i


# ----------------------------------------------------------------------------------------------------------- the restatement
def upsample(d, size, mode="bilinear", align=False):
    if tuple(d.shape[2:]) == tuple(size):
        return d
    if mode == "nearest":
        return F.interpolate(d, size, mode="nearest")
    return F.interpolate(d, size, mode="bilinear", align_corners=align)


def smooth(disp, img):
    """reference layers.py:199-212 (get_smooth_loss); an empty direction contributes 0"""
    gx = (disp[:, :, :, :-1] - disp[:, :, :, 1:]).abs() * torch.exp(-(img[:, :, :, :-1] - img[:, :, :, 1:]).abs().mean(1, keepdim=True))
    gy = (disp[:, :, :-1, :] - disp[:, :, 1:, :]).abs() * torch.exp(-(img[:, :, :-1, :] - img[:, :, 1:, :]).abs().mean(1, keepdim=True))
    zero = disp.sum() * 0
    return (gx.mean() if gx.numel() else zero) + (gy.mean() if gy.numel() else zero)


def colour(tgt, s):
    return tgt if s == 0 else F.interpolate(tgt, (tgt.shape[2] >> s, tgt.shape[3] >> s), mode="area")


def evaluate(tgt, refs, disps, K, inv_K, T, align, automask, smoothness=SMOOTHNESS, weights=None, mutant=None):
    """The objective in the dtype of its inputs -> dict(loss, parts [S,2], sel (list), ev (reproj_audit.evaluate's dict per scale)).
    `mutant`: one of tests/test_mono2_audit_host.py's."""
    S = len(disps)
    h, w = tgt.shape[2:]
    total, parts, sels, evs = 0, [], [], []
    for s, d in enumerate(disps):
        if mutant == "up_align":
            up = upsample(d, (h, w), align=True)
        elif mutant == "up_nearest":
            up = upsample(d, (h, w), mode="nearest")
        else:
            up = upsample(d, (h, w))
        ev = RA.evaluate(tgt, refs, up, K, inv_K, T, align, automask)
        m = ev["m"]
        if mutant == "coarse_identity" and automask and s > 0:
            # the identity terms taken at the resolution of the scale (and brought back by nearest upsampling)
            ct = colour(tgt, s)
            ident = torch.stack([upsample(RA.term(colour(r, s), ct).unsqueeze(1), (h, w), mode="nearest")[:, 0] for r in refs], 0)
            terms = torch.cat([ident, ev["terms"][len(refs):]], 0)
            m = terms.min(0)[0].unsqueeze(1)
        mean = d.mean() if mutant == "batch_mean" else d.mean((2, 3), keepdim=True)
        sm = smooth(d / (mean + 1e-7), colour(tgt, s))
        rep = (m if weights is None else m * weights[s]).mean()
        wgt = smoothness if mutant == "no_scale_weight" else smoothness / 2 ** s
        total = total + rep + wgt * sm
        parts.append(torch.stack([rep, sm]))
        sels.append(ev["sel"])
        evs.append(ev)
    loss = total if mutant == "no_average" else total / S
    return dict(loss=loss, parts=torch.stack(parts), sel=sels, ev=evs)


MUTANTS = ("up_align", "up_nearest", "batch_mean", "no_scale_weight", "no_average", "coarse_identity")


def _args(name, dtype, S):
    i = inputs(name)
    c = lambda t: t.to(dtype)
    return c(i["tgt"]), [c(r) for r in i["refs"]], [c(d) for d in i["disps"][:S]], c(i["K"]), c(i["inv_K"]), [c(t) for t in i["T"]]


# ------------------------------------------------------------------------------------------------------- the fragile pixels
def _fragile_of(tgt, refs, ev, align):
    """reproj_audit.fragile()'s rule on one evaluation (fp64): bool [B,H,W]"""
    b, _, h, w = tgt.shape
    out = torch.zeros((b, h, w), dtype=torch.bool)
    if ev["terms"].shape[0] > 1:
        two = torch.sort(ev["terms"], 0)[0][:2]
        out |= (two[1] - two[0]) < RA.TAU_TIE
    for pred, grid in zip(ev["pred"], ev["grid"]):
        raw = RA.ssim_raw(pred, tgt)
        out |= ((raw.abs() < RA.TAU_SSIM) | ((raw - 1).abs() < RA.TAU_SSIM)).any(1)
        ix, iy = RA.unnormalise(grid[..., 0], w, align), RA.unnormalise(grid[..., 1], h, align)
        near = lambda v, n: ((v - v.round()).abs() < RA.TAU_PX) & (v > -RA.TAU_PX) & (v < n - 1 + RA.TAU_PX)
        kink = ((tgt - pred).abs() < RA.TAU_L1).any(1)
        out |= RA._dilate(near(ix, w) | near(iy, h) | kink)
    return out


@functools.lru_cache(maxsize=None)
def fragile(name, align, automask, S=S_MAX):
    """list of S bool [B,1,H,W] from the fp64 evaluation; asserts the cap for every scale"""
    tgt, refs, disps, K, inv_K, T = _args(name, torch.float64, S)
    ev = evaluate(tgt, refs, disps, K, inv_K, T, align, automask)
    out = []
    for s in range(S):
        f = _fragile_of(tgt, refs, ev["ev"][s], align)
        share = float(f.double().mean())
        assert share <= CAP, "%s scale %d (align %s, automask %s): %.2f %% of the pixels are fragile, cap %.0f %%" % (
            name, s, align, automask, 100 * share, 100 * CAP)
        out.append(f.unsqueeze(1))
    return out


def fragile_shares(name, align, automask, S=S_MAX):
    """the shares fragile() would assert on, without the assert"""
    tgt, refs, disps, K, inv_K, T = _args(name, torch.float64, S)
    ev = evaluate(tgt, refs, disps, K, inv_K, T, align, automask)
    return [float(_fragile_of(tgt, refs, ev["ev"][s], align).double().mean()) for s in range(S)]


def weights(name, align, automask, S=S_MAX):
    """[S,B,1,H,W] fp32: the upstream maps of the gradient comparison (zero on the fragile pixels; all zero for a VALUE case)"""
    i = inputs(name)
    if name in VALUE_CASES:
        return torch.zeros((S,) + tuple(i["g"][0].shape))
    fr = fragile(name, align, automask, S)
    return torch.stack([i["g"][s] * (~fr[s]) for s in range(S)], 0)


# -------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def reference(name, align, automask, dtype, S=S_MAX, mutant=None):
    """dict(loss, parts: unweighted values; sel, near_tie: lists; ddisp (list), dT (list): gradients of the weighted objective)"""
    tgt, refs, disps, K, inv_K, T = _args(name, dtype, S)
    with torch.no_grad():
        val = evaluate(tgt, refs, disps, K, inv_K, T, align, automask, mutant=mutant)
    out = dict(loss=val["loss"], parts=val["parts"], sel=val["sel"])
    near = []
    for ev in val["ev"]:
        nt = torch.zeros_like(ev["sel"], dtype=torch.bool)
        if ev["terms"].shape[0] > 1:
            two = torch.sort(ev["terms"].double(), 0)[0][:2]
            nt = ((two[1] - two[0]) < RA.TAU_TIE).unsqueeze(1)
        near.append(nt)
    out["near_tie"] = near
    if mutant is None:
        dl = [d.clone().requires_grad_(True) for d in disps]
        Tl = [t.clone().requires_grad_(True) for t in T]
        wg = weights(name, align, automask, S).to(dtype)
        evaluate(tgt, refs, dl, K, inv_K, Tl, align, automask, weights=wg)["loss"].backward()
        out["ddisp"], out["dT"] = [d.grad for d in dl], [t.grad for t in Tl]
    return out


def win_shares(name, align, S=S_MAX):
    """per scale the share of the pixels every channel wins (automask), fp64"""
    sel = reference(name, align, True, torch.float64, S)["sel"]
    nch = 2 * CASES[name]["F"]
    return [[float((x == ch).double().mean()) for ch in range(nch)] for x in sel]
