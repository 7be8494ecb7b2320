"""fp64 audit of the supervised-loss, ordinal and error-metric kernels (csrc/dn_loss.hip without smooth2, csrc/dn_ordinal.hip):
the cases, the references as functions of dtype, the fragile-element rule (a plain module, importable without a GPU; the pattern
of geom_audit.py, whose checker and constants it imports).

References.  Every reference is a function of `dtype` evaluated with torch on the CPU: `ref32` is the fp32 oracle (never the
kernel), `ref64` takes the SAME fp32 inputs cast up and the kernels' fp32 constants cast up (c32(1e-3), c32(0.2), c32(1e-8),
c32(1.25 ** 2) ...), so that a threshold is the same number on both sides.  oracle/losses.py supplies the pyramids, the crop bounds,
the maximum depths and the explainability loss; restated here, because the oracle writes them with Python doubles or for fp32 only:
the masked terms (constants, fp32 count in the scale-invariant term), the ordinal head from strided logits, the DORN loss from an
fp32 `ord`, SID, the integer upsample and compute_errors with its lower-middle median.  Two places where torch's autograd is not
the definition: berHu with max r == 0 (torch's `where` sends NaN through its dead branch; the value is mean r and the gradient is
sign(0) = 0), and every reference takes `mutant`, a name from MUTANTS, to produce the deliberately wrong variants that
tests/test_loss_audit_host.py shows the checker to reject.

Inputs.  gt and pred of the masked losses lie on a dyadic grid (multiples of 2^-8 below 128): gt - pred is exact in fp32, so ties
of r, d == 0 and the side of r > c are deliberate and identical in fp32 and fp64.  The clamp bounds themselves (c32(1e-3),
max_depth) are planted as exact values.  Everything comes from oracle.detgen.

Fragile elements are found from the fp64 values and handled BEFORE the comparison: thr within TAU_THR of 1.25^k in compute_errors
(those pixels get gt = 0), P within TAU_P of 0.5 in the ordinal decode (the count may differ by the number of such planes of the
pixel), K log(t) / log(beta) within TAU_SID of an integer (the label may differ by one).  _cap() asserts that a case loses at most
CAP of its elements.

Measured on an MI355X: the worst err / max(max|ref32 - ref64|, FLOOR * max|ref64| / MARGIN) per quantity over all cases and
both forward paths (tests/test_gpu_loss_fp64.py prints every figure) --
  per-sample l1 / l2 / berHu / scale-inv (11 cases x fused and three launches)
                                     loss 2.89 / 2.65 / 2.61 / 1.20   dpred 3.72 / 1.77 / 2.13 / 1.10
                                     (loss: groups_257 and split_cap, 257 group values or 64 split partials added one after the
                                     other by one thread; dpred l1: one_split, where the oracle's error is a single rounding)
  Multiscale_* (8 runs x 2 paths)    loss 4.97 (L1, avg pyramid)   dpred per scale 1.66 (berHu) or 1.00
  upsample_min                       nearest: out exact, dx 1.00   bilinear: out 1.08, dx 1.48 (1x1 x 8: 64 products added)
  explain_edges                      loss 1.18   dmask 1.00 at the edge values, 0.90 inside
  ord_K3 / ord_K8 / ord_K17          ord 1.00   dlogits 0.91 (the two layouts give equal bits)   decode equal on every pixel
                                     DORN loss 7.34 (ord_K3: the plane sum of a thread in fp32, the partials in fp64, against torch's
                                     pairwise sum -- the largest figure of the audit)   dord 1.00
  sid                                labels differ from the fp64 label on 75 - 98 of 16 600 depths, all fragile, all by one;
                                     get_depth_sid 1.00
  errors_median                      abs_diff 2.08  abs_rel 1.00  sq_rel 4.18  rmse 1.00  rmse_log 1.86  a1 a2 a3 1.00; the
                                     medians equal the lower middle of the sorted valid set bit for bit
No quantity needs more than 7.4 of the margin of 16, and none needs an `extra` allowance.  The fused forward and the three launches
give equal bits on every non-berHu case, and two runs of every kernel give equal bits.  No defect was found in the kernels.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from geom_audit import CAP, FLOOR, MARGIN, U, check, compare  # noqa: F401  (the one tolerance rule of the audits)
from oracle import detgen, losses as OL

F64, F32 = torch.float64, torch.float32


def c32(v):
    """the fp32 constant of the kernels as a Python float: the same number in an fp32 and in an fp64 expression"""
    return float(np.float32(v))


LO = c32(1e-3)                 # clamp of the prediction
C02 = c32(0.2)                 # berHu: c = 0.2 max r
EPS, BIG = c32(1e-8), c32(1e8)  # clamp of the ordinal logits and of P / 1 - P
MAXD = 80.0                    # 'kitti'; every masked case runs with it
THR = (c32(1.25), c32(1.25 * 1.25), c32(1.25 * 1.25 * 1.25))
TAU_THR = 1e-6                 # relative: fp32 forms thr with two quotients and a product by the median ratio, <= 4 U relative
TAU_P = 1e-6                   # |P - 0.5|: fp32 forms P with two exps, a sum and a quotient, <= 4 U
TAU_SID = 4e-5                 # |v - round(v)|: v <= 80 carries <= 4 U v + K / log(beta) U = 2.3e-5 in fp32
KINDS = ("l1", "l2", "berhu", "scale_inv")
LOSS_SPLIT_PIXELS, LOSS_SPLIT_MAX = 2048, 64          # loss_splits() of dn_loss.hip
BWD_GRID_ELEMS = 4096 * 256                           # masked_loss_bwd_kernel's grid cap
REDUCE1D_ELEMS = 1024 * 256                           # dn_reduce1d_blocks' cap
FOLD_GROUPS = 256                                     # kFoldLossGroups

MUTANTS = ("valid_le_max", "clamp_passes", "berhu_tie_whole", "berhu_no_c_path", "si_factor", "mean_all", "whole_batch",
           "weights_swapped", "k_le_t", "ord_clamp_passes", "one_minus_p_unclamped", "upper_median", "align_corners", "strides_swapped")


def loss_splits(pixels):
    return max(1, min(LOSS_SPLIT_MAX, (pixels + LOSS_SPLIT_PIXELS - 1) // LOSS_SPLIT_PIXELS))


def _cap(name, n_fragile, n_total):
    share = n_fragile / float(max(n_total, 1))
    assert share <= CAP, "%s: %.2f %% of the elements are fragile, cap %.0f %%" % (name, 100 * share, 100 * CAP)
    return share


def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------------------------------ inputs
def grid(shape, tag, lo, hi):
    """multiples of 2^-8 in [lo, hi), |values| < 128: exact in fp32, and so are their differences"""
    return torch.floor(detgen.uniform(shape, tag, lo, hi, dtype=torch.float64) * 256).div(256).float()


def pick(shape, tag, n):
    """an integer 0 .. n-1 per element (equal shares)"""
    return torch.floor(detgen.uniform(shape, tag, 0, n, dtype=torch.float64)).long()


# name -> (B, h, w) of the per-sample cases (G = B groups of h * w pixels)
MASKED_CASES = {
    "one_split": (3, 5, 7),
    "two_splits": (2, 3, 683),             # 2049 pixels
    "split_cap": (1, 257, 503),            # 129 271 pixels > 63 * 2048: 64 splits
    "bwd_grid_cap": (2, 600, 900),         # 1 080 000 elements > 4096 * 256: a second trip of the backward's grid stride (gradient only)
    "groups_256": (256, 5, 7),             # the last size of the fused forward
    "groups_257": (257, 5, 7),             # the first size that must take the three launches
    "clamp_edges": (2, 9, 13),
    "l1_zero_diff": (2, 9, 13),
    "empty_group": (3, 5, 7),
    "berhu_ties": (3, 5, 7),
    "berhu_flat": (2, 5, 7),
}
TIE_COUNTS = (1, 2, 5)
TIE_POS = (3, 17, 20, 29, 34)
TIE_R = 8.0                                # the planted maximum of r; every other r is below 4, on both sides of c = 1.6


@functools.lru_cache(maxsize=None)
def masked_inputs(name):
    """(gt [B, h, w], pred [B, 1, h, w]) in fp32"""
    b, h, w = MASKED_CASES[name]
    tag, s = "loss:" + name, (b, h, w)
    gt = grid(s, tag + ":gt", 0.5, 79.75)
    pred = grid(s, tag + ":pred", 0.5, 79.75)
    if name == "clamp_edges":
        # pred: an eighth each below 1e-3 (0 and negatives included), exactly c32(1e-3), exactly max_depth, above it; gt: an eighth
        # each exactly 0 and exactly max_depth (both invalid)
        p = pick(s, tag + ":psel", 8)
        pred = torch.where(p == 0, grid(s, tag + ":below", -2.0, 2.0 ** -8), pred)
        pred = torch.where(p == 1, torch.full(s, LO), pred)
        pred = torch.where(p == 2, torch.full(s, MAXD), pred)
        pred = torch.where(p == 3, grid(s, tag + ":above", MAXD + 2.0 ** -8, 95.0), pred)
        g = pick(s, tag + ":gsel", 8)
        gt = torch.where(g == 0, torch.zeros(s), gt)
        gt = torch.where(g == 1, torch.full(s, MAXD), gt)
    elif name == "l1_zero_diff":
        pred = torch.where(pick(s, tag + ":same", 4) == 0, gt, pred)
        gt = gt * (pick(s, tag + ":inv", 5) != 0)
    elif name == "berhu_ties":
        gt = grid(s, tag + ":gt", 10.0, 60.0)
        pred = gt + grid(s, tag + ":delta", -3.75, 3.75)
        for i, n in enumerate(TIE_COUNTS):
            for j, pos in enumerate(TIE_POS[:n]):
                pred.view(b, -1)[i, pos] = gt.view(b, -1)[i, pos] + (TIE_R if j % 2 == 0 else -TIE_R)
    elif name == "berhu_flat":
        inv = pick(s, tag + ":inv", 4) == 0
        pred = torch.where(inv, pred, gt)
        gt = gt * ~inv
    else:
        # a fifth of gt invalid (0, exactly max_depth, above), a tenth of pred below and a tenth above the clamp
        g = pick(s, tag + ":gsel", 15)
        gt = torch.where(g == 0, torch.zeros(s), gt)
        gt = torch.where(g == 1, torch.full(s, MAXD), gt)
        gt = torch.where(g == 2, grid(s, tag + ":gabove", MAXD, 90.0), gt)
        p = pick(s, tag + ":psel", 10)
        pred = torch.where(p == 0, grid(s, tag + ":below", -2.0, 2.0 ** -8), pred)
        pred = torch.where(p == 1, grid(s, tag + ":above", MAXD + 2.0 ** -8, 95.0), pred)
        if name == "empty_group":
            gt[1] = 0
    return gt, pred.reshape(b, 1, h, w)


def masked_shares(name):
    """what the host test asserts on: splits, backward elements, shares of the clamp / validity edges, tie counts (all exact: the grid)"""
    gt, pred = masked_inputs(name)
    b, h, w = gt.shape
    p = pred.reshape(b, h, w)
    valid = (gt > 0) & (gt < MAXD)
    f = lambda m: float(m.double().mean())
    r = ((gt - p.clamp(LO, MAXD)).abs() * valid).reshape(b, -1)
    mx = r.max(1, keepdim=True).values
    return dict(groups=b, pixels=h * w, splits=loss_splits(h * w), elems=b * h * w, valid=f(valid),
                pred_below=f(p < LO), pred_lo=f(p == LO), pred_hi=f(p == MAXD), pred_above=f(p > MAXD),
                gt_zero=f(gt == 0), gt_max=f(gt == MAXD), gt_above=f(gt > MAXD), zero_diff=f(valid & (gt == p)),
                ties=[int(t) for t in ((r == mx) & valid.reshape(b, -1)).sum(1)], max_r=[float(m) for m in mx[:, 0]],
                above_c=f((r > C02 * mx) & valid.reshape(b, -1)), empty=[int(i) for i in range(b) if not bool(valid[i].any())])


# ------------------------------------------------------------------------------------------------- masked-loss references
def masked_term(kind, gt, pred, max_depth, mutant=None):
    """one group: gt, pred of equal shape in one dtype (pred may require grad) -> the group's loss"""
    valid = (gt > 0) & ((gt <= max_depth) if mutant == "valid_le_max" else (gt < max_depth))
    g, pv = gt[valid], pred[valid]
    if mutant == "clamp_passes":           # the clamped value, the gradient of the identity
        p = pv + (pv.detach().clamp(LO, max_depth) - pv.detach())
    else:
        p = pv.clamp(LO, max_depth)
    d = g - p
    mean = (lambda t: t.sum() / gt.numel()) if mutant == "mean_all" else (lambda t: t.mean())
    if kind == "l1":
        return mean(d.abs())
    if kind == "l2":
        return mean(d * d)
    if kind == "berhu":
        r = d.abs()
        if r.numel() == 0 or float(r.detach().max()) == 0.0:
            return mean(r)                 # c = 0: no pixel has r > c, the value is mean r (module docstring)
        mx = r.max()
        if mutant == "berhu_no_c_path":
            mx = mx.detach()
        elif mutant == "berhu_tie_whole":  # every tied pixel gets the whole gradient of the maximum
            n_tie = (r.detach() == mx.detach()).sum()
            mx = mx.detach() + (mx - mx.detach()) * n_tie
        c = C02 * mx
        return mean(torch.where(r > c, (r * r + c * c) / (2 * c), r))
    if kind == "scale_inv":
        n = torch.tensor(float(g.numel()), dtype=pred.dtype)
        return mean((g.abs() - p.abs()) ** 2) - (1.0 if mutant == "si_factor" else 0.5) * d.sum() ** 2 / (n * n)
    raise ValueError(kind)


def masked_reference(kind, terms, max_depth, dtype, mutant=None):
    """terms: [(gt, pred, groups, weight)], fp32 tensors; the loss is sum_i weight_i * mean over the groups of term i, added in term and
    group order like the kernels' finalize.  Returns (loss, [dpred per term])."""
    if mutant == "weights_swapped":
        ws = [t[3] for t in terms][::-1]
        terms = [(g, p, n, w) for (g, p, n, _), w in zip(terms, ws)]
    leaves, total = [], None
    for gt, pred, groups, weight in terms:
        p = _leaf(pred, dtype)
        leaves.append(p)
        if mutant == "whole_batch":
            groups = 1
        gg, pp = gt.to(dtype).reshape(groups, -1), p.reshape(groups, -1)
        s = None
        for k in range(groups):
            t = masked_term(kind, gg[k], pp[k], max_depth, mutant)
            s = t if s is None else s + t
        v = weight * (s / groups)
        total = v if total is None else total + v
    total.backward()
    return total.detach(), [p.grad if p.grad is not None else torch.zeros_like(p) for p in leaves]


@functools.lru_cache(maxsize=None)
def per_sample_reference(name, kind, dtype, mutant=None):
    """(loss, dpred [B, 1, h, w]) of l1_loss / l2_loss / berhu_loss / Scale_invariant_loss ('kitti') on a MASKED_CASES case"""
    gt, pred = masked_inputs(name)
    loss, (g,) = masked_reference(kind, [(gt, pred, gt.shape[0], 1.0)], MAXD, dtype, mutant)
    return loss, g


# ------------------------------------------------------------------------------------------------------------ multiscale
MULTISCALE = dict(B=2, sizes=((24, 40), (12, 20), (6, 10), (3, 5)))
# (public function, its pool_type or None, kind)
MULTISCALE_RUNS = (("Multiscale_L1_loss", "max", "l1"), ("Multiscale_L1_loss", "avg", "l1"), ("Multiscale_L1_loss", "bilinear", "l1"),
                   ("Multiscale_L2_loss", None, "l2"), ("Multiscale_berhu_loss", None, "berhu"), ("Multiscale_scale_inv_loss", None, "scale_inv"),
                   ("Multiscale_FULL_L1_loss", "nearest", "l1"), ("Multiscale_FULL_L1_loss", "bilinear", "l1"))


@functools.lru_cache(maxsize=None)
def multiscale_inputs():
    """gt [B, 24, 40] (two fifths are 0; one in a hundred is max_depth or above -- few, because the max pyramid spreads them over 8 x 8
    blocks and the coarsest scale must keep valid pixels) and the four predictions [B, 1, h, w], all on the dyadic grid -- and so
    are the three pyramids (sums of four grid values times 1/4 stay exact in fp32 for three levels)"""
    b, (h, w) = MULTISCALE["B"], MULTISCALE["sizes"][0]
    tag, s = "loss:multiscale", (b, h, w)
    gt = grid(s, tag + ":gt", 0.5, 79.75)
    g = pick(s, tag + ":gsel", 200)
    gt = torch.where(g < 80, torch.zeros(s), gt)
    gt = torch.where(g == 80, torch.full(s, MAXD), gt)
    gt = torch.where(g == 81, grid(s, tag + ":gabove", MAXD, 90.0), gt)
    preds = []
    for i, (hh, ww) in enumerate(MULTISCALE["sizes"]):
        ss = (b, 1, hh, ww)
        p = grid(ss, tag + ":pred%d" % i, 0.5, 79.75)
        sel = pick(ss, tag + ":psel%d" % i, 10)
        p = torch.where(sel == 0, grid(ss, tag + ":below%d" % i, -2.0, 2.0 ** -8), p)
        p = torch.where(sel == 1, grid(ss, tag + ":above%d" % i, MAXD + 2.0 ** -8, 95.0), p)
        preds.append(p)
    return gt, preds


def upsample_ref(x, scale, mode, mutant=None):
    """F.upsample(scale_factor, mode) as Multiscale_FULL_L1_loss calls it: nearest, or bilinear with align_corners=False"""
    if mode == "nearest":
        return F.interpolate(x, scale_factor=scale, mode="nearest")
    return F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=(mutant == "align_corners"))


@functools.lru_cache(maxsize=None)
def multiscale_reference(fn, pool, kind, dtype, mutant=None):
    """(loss, [dpred per scale]) of the public Multiscale_* function `fn`: whole-batch groups, weights 1 / 2^i, max depth 80"""
    gt, preds = multiscale_inputs()
    leaves = [_leaf(p, dtype) for p in preds]
    if fn == "Multiscale_FULL_L1_loss":
        gts = [gt.to(dtype)] * len(preds)
        ps = [upsample_ref(p, 2 ** i, pool, mutant) for i, p in enumerate(leaves)]
    else:
        gts = OL._gt_pyramid(gt.to(dtype), pool or "bilinear")
        ps = leaves
    ws = [1.0 / 2 ** i for i in range(len(ps))]
    if mutant == "weights_swapped":
        ws = ws[::-1]
    total = None
    for g, p, w in zip(gts, ps, ws):
        v = w * masked_term(kind, g.reshape(-1), p.reshape(-1), 80.0, mutant)
        total = v if total is None else total + v
    total.backward()
    return total.detach(), [p.grad for p in leaves]


# -------------------------------------------------------------------------------------------------------------- upsample
UPSAMPLE = dict(planes=(2, 3), sizes=((1, 1), (1, 3), (2, 2), (3, 5)), scales=(1, 2, 4, 8), modes=("nearest", "bilinear"))


def upsample_inputs(size, scale):
    b, c = UPSAMPLE["planes"]
    tag = "loss:upsample:%dx%d:x%d" % (size + (scale,))
    return (detgen.uniform((b, c) + size, tag + ":x", -1, 1),
            detgen.uniform((b, c, size[0] * scale, size[1] * scale), tag + ":g", -1, 1))


@functools.lru_cache(maxsize=None)
def upsample_reference(size, scale, mode, dtype, mutant=None):
    x, g = upsample_inputs(size, scale)
    xl = _leaf(x, dtype)
    out = upsample_ref(xl, scale, mode, mutant)
    (out * g.to(dtype)).sum().backward()
    return out.detach(), xl.grad


# -------------------------------------------------------------------------------------------------------- explainability
EXPLAIN_SIZES = (1, 257, REDUCE1D_ELEMS + 300)          # one element; two blocks, the second partial; past the block cap of the reduction
EXPLAIN_EDGE_VALUES = (1.0, 0.0, 1e-44, 1e-20, 1e-13)   # log(1) = 0 and a zero gradient | log clamps at -100 (twice) | (1 - x) x < 1e-12 (all four)


@functools.lru_cache(maxsize=None)
def explain_inputs(n):
    """mask [1, 1, 1, n] and `edge` (bool): a quarter of the elements take EXPLAIN_EDGE_VALUES in equal shares; n == 1 is the value 1e-13.  The
    gradient at the edge values is 1e12 times the interior's, so the two sets are compared separately."""
    tag = "loss:explain:%d" % n
    m = detgen.uniform((n,), tag, 0.05, 0.95)
    sel = pick((n,), tag + ":sel", 4 * len(EXPLAIN_EDGE_VALUES))
    edge = sel < len(EXPLAIN_EDGE_VALUES)
    vals = torch.tensor(EXPLAIN_EDGE_VALUES, dtype=torch.float32)
    m = torch.where(edge, vals[sel.clamp(max=len(vals) - 1)], m)
    if n == 1:
        m, edge = torch.tensor([1e-13]), torch.tensor([True])
    return m.reshape(1, 1, 1, n), edge.reshape(1, 1, 1, n)


@functools.lru_cache(maxsize=None)
def explain_reference(n, dtype):
    m, _ = explain_inputs(n)
    ml = _leaf(m, dtype)
    v = OL.explainability_loss(ml)          # ATen's binary_cross_entropy: -max(log, -100), backward (x - 1) / max((1 - x) x, 1e-12)
    v.backward()
    return v.detach(), ml.grad


# --------------------------------------------------------------------------------------------------------------- ordinal
ORD_CASES = {"ord_K3": 3, "ord_K8": 8, "ord_K17": 17}     # below the 8-plane unroll | exactly one trip | two trips and a tail of one
ORD_N, ORD_H, ORD_W = 2, 7, 11
LAYOUTS = ("nchw", "nhwc")


@functools.lru_cache(maxsize=None)
def ordinal_inputs(name):
    """logits [N, 2K, H, W] (logical NCHW, contiguous), the upstream dord [N, K, H, W], gt [N, H, W] (a quarter invalid) and the
    targets [N, H, W] int32 over 0, mid, K and K + 3.  Of the logits an eighth is negative, a sixteenth each is in [0, 1e-8) (exact
    zeros included) and above 1e8; of the (A, B) pairs an eighth is more than 20 apart, half of them each way."""
    k = ORD_CASES[name]
    tag, s = "loss:" + name, (ORD_N, 2 * k, ORD_H, ORD_W)
    x = detgen.uniform(s, tag + ":x", 0.0, 6.0)
    sel = pick(s, tag + ":sel", 16)
    x = torch.where(sel <= 1, detgen.uniform(s, tag + ":neg", -5.0, 0.0), x)
    x = torch.where(sel == 2, detgen.uniform(s, tag + ":tiny", 0.0, 2e-8) - 1e-8, x).clamp(min=-5.0)
    x = torch.where((sel == 2) & (x < 0), torch.zeros(s), x)
    x = torch.where(sel == 3, torch.full(s, 3e8), x)
    ps = (ORD_N, k, ORD_H, ORD_W)
    far = pick(ps, tag + ":far", 16)
    a, b = x[:, 0::2].clone(), x[:, 1::2].clone()
    spread = detgen.uniform(ps, tag + ":spread", 21.0, 40.0)
    a = torch.where(far == 0, torch.full(ps, 0.5), a)
    b = torch.where(far == 0, 0.5 + spread, b)
    b = torch.where(far == 1, torch.full(ps, 0.5), b)
    a = torch.where(far == 1, 0.5 + spread, a)
    x = torch.stack((a, b), 2).reshape(s).contiguous()
    gs = (ORD_N, ORD_H, ORD_W)
    gt = grid(gs, tag + ":gt", 0.5, 79.75) * (pick(gs, tag + ":inv", 4) != 0)
    target = torch.tensor([0, k // 2, k, k + 3], dtype=torch.int32)[pick(gs, tag + ":t", 4)]
    return x, detgen.uniform(ps, tag + ":g", -1, 1), gt, target


def ordinal_head(x, mutant=None):
    """OrdinalRegressionLayer on logical NCHW logits of any dtype: P = softmax(clamp(A), clamp(B))[1], [N, K, H, W]"""
    a, b = x[:, 0::2], x[:, 1::2]
    if mutant == "ord_clamp_passes":
        a, b = (t + (t.detach().clamp(EPS, BIG) - t.detach()) for t in (a, b))
    else:
        a, b = a.clamp(EPS, BIG), b.clamp(EPS, BIG)
    return torch.softmax(torch.stack((a, b), 0), 0)[1]


@functools.lru_cache(maxsize=None)
def ordinal_reference(name, dtype, mutant=None):
    """(ord, decode [N, 1, H, W] int64, dlogits) under the case's upstream gradient"""
    x, g, _, _ = ordinal_inputs(name)
    xl = _leaf(x, dtype)
    p = ordinal_head(xl, mutant)
    (p * g.to(dtype)).sum().backward()
    grad = xl.grad
    if mutant == "strides_swapped":     # the gradient of logical (n, c, p) written where an NHWC buffer read as NCHW puts it
        n, c2, h, w = grad.shape
        grad = grad.permute(0, 2, 3, 1).contiguous().view(n, c2, h, w)
    return p.detach(), (p.detach() > 0.5).sum(1, keepdim=True), grad


@functools.lru_cache(maxsize=None)
def decode_fragile(name):
    """planes whose fp64 P lies within TAU_P of 0.5 and is not exactly 0.5 (both logits clamped to 1e-8 give exactly 0.5 in either
    precision): bool [N, K, H, W]; the decode may differ by their number per pixel"""
    p = ordinal_reference(name, F64)[0]
    frag = ((p - 0.5).abs() < TAU_P) & (p != 0.5)
    _cap(name + ":decode", int(frag.sum()), frag.numel())
    return frag


@functools.lru_cache(maxsize=None)
def ordinal_prob32(name):
    """the fp32 `ord` that the DORN-loss cases take as their INPUT (the fp32 oracle's, so that it exists without a GPU)"""
    return ordinal_reference(name, F32)[0].contiguous()


def dorn_loss_ref(ord_, gt, target, max_depth, mutant=None):
    n, k, h, w = ord_.shape
    valid = ((gt > 0) & (gt < max_depth)).unsqueeze(1)
    kk = torch.arange(k, dtype=torch.int32).view(1, k, 1, 1)
    t = target.unsqueeze(1).to(torch.int32)
    le = (kk <= (t if mutant == "k_le_t" else t - 1))
    q = 1 - ord_
    lp = torch.log(ord_.clamp(EPS, BIG))
    lq = torch.log(q if mutant == "one_minus_p_unclamped" else q.clamp(EPS, BIG))
    s = (torch.where(le, lp, lq) * valid).sum()
    return s / (-valid.sum().to(ord_.dtype))


@functools.lru_cache(maxsize=None)
def dorn_reference(name, dtype, mutant=None):
    """(loss, dord) of DORN_loss('kitti') from the fp32 ord of ordinal_prob32()"""
    _, _, gt, target = ordinal_inputs(name)
    o = _leaf(ordinal_prob32(name), dtype)
    v = dorn_loss_ref(o, gt.to(dtype), target, MAXD, mutant)
    v.backward()
    return v.detach(), o.grad


def dorn_shares(name):
    x, _, gt, target = ordinal_inputs(name)
    p = ordinal_prob32(name)
    k = p.shape[1]
    f = lambda m: float(m.double().mean())
    return dict(neg=f(x < 0), tiny=f((x >= 0) & (x < EPS)), big=f(x > BIG), p_small=f(p < EPS), q_zero=f((1 - p) == 0),
                q_small=f((1 - p) < EPS), invalid=f(~((gt > 0) & (gt < MAXD))),
                targets=sorted(set(int(t) for t in target.reshape(-1))), K=k)


# ------------------------------------------------------------------------------------------------------------------- SID
SID_CASES = ((71.0, "kitti"), (80.0, "kitti"), (80.0, "nyu"))
SID_SWEEP = 16384


def sid_beta(dataset):
    return c32({"kitti": 80.999, "nyu": 10.999}[dataset])


@functools.lru_cache(maxsize=None)
def sid_inputs(k, dataset):
    """depths (fp32): a log-spaced sweep over the dataset's range, 0 and a few depths below the first edge (v < 0 truncates toward 0,
    not down), and for every bin edge beta^(l / K) - 0.999 the nearest fp32 depth and its two neighbours"""
    beta = sid_beta(dataset)
    mx = OL.MAX_DEPTH[dataset]
    sweep = np.exp(np.linspace(np.log(1e-3), np.log(mx), SID_SWEEP)).astype(np.float32)
    edges = (np.power(beta, np.arange(0, int(k) + 1) / k) - 0.999).astype(np.float32)
    below = np.nextafter(edges, np.float32(-np.inf))
    above = np.nextafter(edges, np.float32(np.inf))
    d = np.concatenate([sweep, np.zeros(1, np.float32), edges, below, above])
    return torch.from_numpy(d[d >= 0])


def sid_value(depth, k, dataset, dtype):
    """K log(depth + 0.999) / log(beta) before the truncation, in dtype (fp32 constants)"""
    d = depth.to(dtype)
    return (k * torch.log(d + c32(0.999))) / torch.log(torch.tensor(sid_beta(dataset), dtype=dtype))


@functools.lru_cache(maxsize=None)
def sid_reference(k, dataset):
    """(labels int32 from the fp64 value, fragile bool): a fragile label may differ by one"""
    v = sid_value(sid_inputs(k, dataset), k, dataset, F64)
    frag = (v - v.round()).abs() < TAU_SID
    _cap("sid:%g:%s" % (k, dataset), int(frag.sum()), frag.numel())
    return v.trunc().to(torch.int32), frag


def sid_depth_ref(labels, k, dataset, dtype):
    l = labels.to(dtype)
    beta = torch.tensor(sid_beta(dataset), dtype=dtype)
    return 0.5 * (beta ** (l / k) + beta ** ((l + 1.0) / k)) - c32(0.999)


# -------------------------------------------------------------------------------------------------------- compute_errors
ERRORS = dict(B=3, h=37, w=53)          # 'kitti' with the Garg crop: rows 15:36, columns 1:51
METRICS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def crop_mask(h, w, crop):
    m = torch.zeros(h, w, dtype=torch.bool)
    y1, y2, x1, x2 = OL.garg_crop_bounds(h, w) if crop else (0, h, 0, w)
    m[y1:y2, x1:x2] = True
    return m


def lower_median(v, mutant=None):
    s = v.sort().values
    return s[s.numel() // 2 if mutant == "upper_median" else (s.numel() - 1) // 2]


def errors_ref(gt, pred, dtype, crop=True, unsupervised=True, mutant=None):
    """compute_errors('kitti') in dtype: ([8 metrics], medians [B, 2], thr per sample) -- the kernel's operation order where it matters
    (pred * median(gt) / median(pred)), the mean over the batch of the per-sample values"""
    b, h, w = gt.shape
    cm = crop_mask(h, w, crop)
    acc, meds, thrs = torch.zeros(8, dtype=dtype), [], []
    for g, p in zip(gt.to(dtype), pred.to(dtype)):
        valid = (g > 0) & (g < MAXD) & cm
        vg, vp = g[valid], p[valid].clamp(LO, MAXD)
        mg, mp = lower_median(vg, mutant), lower_median(vp, mutant)
        meds.append(torch.stack((mg, mp)))
        if unsupervised:
            vp = vp * mg / mp
        thr = torch.max(vg / vp, vp / vg)
        d = vg - vp
        dl = torch.log(vg) - torch.log(vp)
        terms = [d.abs().mean(), (d.abs() / vg).mean(), (d * d / vg).mean(), (d * d).mean().sqrt(), (dl * dl).mean().sqrt()]
        terms += [(thr < t).to(dtype).mean() for t in THR]
        acc = acc + torch.stack(terms)
        thrs.append((valid, thr))
    return acc / b, torch.stack(meds), thrs


@functools.lru_cache(maxsize=None)
def errors_inputs(unsupervised=True):
    """(gt [B, h, w], pred [B, h, w], n_removed): sample 0 has an even and sample 1 an odd number of valid pixels inside the crop,
    sample 2 exactly one.  In sample 0 a third of the predictions lies below 1e-3 and a third above max_depth (the select walks past
    two heavily tied values); in sample 1 three fifths lie above max_depth, so that the median IS the tied value max_depth.  Pixels
    whose fp64 thr lies within TAU_THR (relative) of 1.25^k are made invalid (gt = 0), again until none is left: the medians move
    when a pixel leaves."""
    b, h, w = ERRORS["B"], ERRORS["h"], ERRORS["w"]
    tag, s = "loss:errors", (b, h, w)
    gt = grid(s, tag + ":gt", 0.5, 79.75) * (pick(s, tag + ":inv", 4) != 0)
    pred = gt * detgen.uniform(s, tag + ":ratio", 0.7, 1.45)          # thr on both sides of all three thresholds
    sel = pick(s, tag + ":psel", 15)
    sel[1] = torch.where(sel[1] >= 6, sel[1], torch.full_like(sel[1], 5))      # sample 1: 0-5 (two fifths) inside, 6-14 above
    sel[0] = sel[0] // 5 * 5                                                   # sample 0: thirds (0 below, 5 inside, 10 above)
    sel[2] = 5
    pred = torch.where(sel == 0, detgen.uniform(s, tag + ":below", -1.0, 1e-3), pred)
    pred = torch.where(sel >= 6, detgen.uniform(s, tag + ":above", MAXD, 95.0), pred)
    cm = crop_mask(h, w, True)
    one = torch.zeros(h, w, dtype=torch.bool)
    one[20, 30] = True
    gt[2] = torch.where(one, torch.tensor(12.5), torch.tensor(0.0))
    pred[2, 20, 30] = 9.75
    removed = 0
    for _ in range(8):
        count = lambda i: int(((gt[i] > 0) & (gt[i] < MAXD) & cm).sum())
        if count(0) % 2 == 1 or count(1) % 2 == 0:       # parity: drop the first valid pixel inside the crop
            i = 0 if count(0) % 2 == 1 else 1
            idx = ((gt[i] > 0) & (gt[i] < MAXD) & cm).reshape(-1).nonzero()[0]
            gt[i].view(-1)[idx] = 0
            continue
        _, _, thrs = errors_ref(gt, pred, F64, True, unsupervised)
        n_new = 0
        for i, (valid, thr) in enumerate(thrs):
            near = torch.zeros_like(thr, dtype=torch.bool)
            for t in THR:
                near |= (thr - t).abs() < TAU_THR * t
            idx = valid.reshape(-1).nonzero()[:, 0][near]
            gt[i].view(-1)[idx] = 0
            n_new += int(near.sum())
        removed += n_new
        _cap("errors_median", removed, int(cm.sum()) * b)
        if n_new == 0:
            break
    else:
        raise AssertionError("errors_median: fragile pixels keep appearing")
    return gt, pred, removed


def errors_counts(unsupervised=True):
    gt, pred, removed = errors_inputs(unsupervised)
    cm = crop_mask(ERRORS["h"], ERRORS["w"], True)
    valid = (gt > 0) & (gt < MAXD) & cm
    p = pred[valid]
    return dict(counts=[int(v.sum()) for v in valid], removed=removed, clamped_lo=float((p < LO).double().mean()),
                clamped_hi=float((p > MAXD).double().mean()))
