"""fp64 audit of the monodepth2 self-supervision kernels (csrc/dn_reproj.hip): the cases, the torch restatement of the reference's
layers.py geometry and of the per-pixel minimum-reprojection loss composed from it, the fragile-pixel rule and the tolerance (a plain
module, importable without a GPU; the pattern of geom_audit.py, whose compare / check / MARGIN / FLOOR it uses unchanged).

The yardstick of loss_functions.min_reprojection_loss is this composition, evaluated by torch on the CPU in fp64 (`ref64`) and in
fp32 (`ref32`):
    depth  = 1 / (1/max_depth + (1/min_depth - 1/max_depth) * disp)
    grid_f = Project3D(BackprojectDepth(depth, inv_K), K, T[f]);  pred_f = grid_sample(ref_imgs[f], grid_f, bilinear, border)
    r_f    = w * SSIM(pred_f, tgt).mean(1) + (1 - w) * |tgt - pred_f|.mean(1);   i_f likewise with ref_imgs[f] for pred_f
    m      = min over [i_0 .. i_{F-1}, r_0 .. r_{F-1}]  (a tie goes to the lowest index);  loss = m.mean()
and the tolerance is geom_audit's measured rule: |got - ref64| <= MARGIN * max|ref32 - ref64| + FLOOR * max|ref64|, the same for the
relative L2 error, MARGIN = 16.

The loss and m are continuous in everything and are compared on all pixels.  The gradients are not: the minimum switches channel
at a tie, SSIM's clamp gates at 0 and 1, the bilinear footprint changes at every integer ix / iy (the border clip included) and
|tgt - pred| has a kink at 0.  An fp32 evaluation may land on the other side of such a point than fp64 does, and both are right.
Those pixels are found from the fp64 evaluation (fragile()) and the upstream map of the reduction="none" form is ZERO there, so
that neither side's gradient sees them; a warped pixel's value reaches the SSIM windows of its 3x3 neighbourhood, so the last two
conditions are dilated by 3x3.  A case may lose at most CAP = 12 % of its pixels this way: a condition on the inputs, not a
measurement -- a case that exceeds it gets other inputs, never another cap.

Measured on an MI355X (tests/test_gpu_reproj.py prints every figure): the worst err / max(max|ref32 - ref64|, FLOOR * max|ref64| /
MARGIN) per quantity over the five loss cases x align_corners x automask --
  m 0.06 (the kernel's SSIM statistics are centred sums: 16 x closer to fp64 than the restatement's E[xy] - mu_x mu_y)   ddisp 1.0   dT 1.7
  loss 7.0 (1x40x136, no automask: a scalar whose fp32 restatement happens to land 3e-9 from fp64 -- 0.43 of the tolerance)
  transformation_from_parameters 1.5   BackprojectDepth / Project3D 1.2, their gradients 1.1   PoseCNN's outputs 1.6
No quantity needs more than 0.43 of the margin of 16.
"""
import functools
import math

import torch
import torch.nn.functional as F

from geom_audit import FLOOR, MARGIN, check, compare  # noqa: F401  (re-exported: the one tolerance rule of the geometry audits)
from oracle import detgen

CAP = 0.12                    # a case may leave out at most this share of its pixels
TAU_TIE = 1e-4                # fragile: gap between the two smallest channels
TAU_SSIM = 1e-4               # fragile: an SSIM term this close to its clamp at 0 or 1
TAU_PX = 1e-3                 # fragile (3x3): ix / iy this close to an integer
TAU_L1 = 1e-5                 # fragile (3x3): |tgt - pred| in some colour plane
MIN_WIN = 0.05                # selection case: every channel wins at least this share of the pixels
TILE_H, TILE_W = 8, 32        # the output tile of a block of the fused kernels (csrc/dn_reproj.hip: kTH, kTW)
MIN_DEPTH, MAX_DEPTH, SSIM_W = 0.1, 100.0, 0.85

ALIGNS = (False, True)
AUTOMASKS = (True, False)

CASES = {
    # the smallest maps ReflectionPad2d(1) accepts
    "min_2x2": dict(B=1, H=2, W=2, F=1, shift=((0.4, 0.3),), trans=0.15, rot=0.02, pert=0.6),
    "min_3x3": dict(B=1, H=3, W=3, F=1, shift=((0.4, -0.3),), trans=0.15, rot=0.2, pert=0.6),
    # ragged against the 8 x 32 tile, and the selection case: every one of the four channels wins its share
    "select_ragged": dict(B=3, H=23, W=37, F=2, shift=((1.6, 0.4), (-1.2, -0.7)), trans=0.05, rot=0.01, select=True),
    # 5 x 5 tiles: tile seams and the image-border reflection in both directions
    "seams": dict(B=1, H=40, W=136, F=2, shift=((1.3, 0.5), (-0.8, 0.9)), trans=0.05, rot=0.01),
    # large motion: coordinates far outside the image (the border clip), points behind the camera (no clamp on c[2])
    "large_motion": dict(B=2, H=23, W=37, F=3, shift=((1.0, 0.0), (0.0, 1.0), (-1.0, 0.5)), trans=0.8, rot=0.35, tz=(-2.6, -0.3, 0.4)),
    # two identical source frames under identical T: exact ties between channel f and f + 1 everywhere
    "twins": dict(B=2, H=11, W=19, F=2, shift=((1.1, 0.3), (1.1, 0.3)), trans=0.05, rot=0.01, twins=True),
}
LOSS_CASES = ("min_2x2", "min_3x3", "select_ragged", "seams", "large_motion")
POSE_CASE = dict(B=5, angle=3.0)
GEOM_SIZES = ((2, 2), (3, 5), (23, 37))


# ------------------------------------------------------------------------------------------------------------------ inputs
def intrinsics(b, h, w):
    """KITTI's intrinsics scaled to h x w as 4x4 matrices (fp32) and their inverse (inverted in fp64, rounded once)."""
    fx, fy, cx, cy = 241.67 * w / 416, 246.28 * h / 128, 204.17 * w / 416, 59.0 * h / 128
    k = torch.tensor([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32).repeat(b, 1, 1)
    return k, torch.inverse(k.double()).float().contiguous()      # (torch.inverse hands out column-major matrices)


def pattern(b, h, w, tag, shift=(0.0, 0.0)):
    """A smooth 3-plane image in (0.1, 0.9): sums of sinusoids with closed-form phases, evaluated at (x - shift_x, y - shift_y), so that
    a shifted copy is exact and not a resampling.  fp64."""
    y = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1) - shift[1]
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w) - shift[0]
    ph = detgen.uniform((b, 3, 4), tag, 0.0, 2 * math.pi, dtype=torch.float64)
    out = 0.5
    for k, (fx, fy, amp) in enumerate(((0.23, 0.11, 0.16), (-0.09, 0.31, 0.12), (0.41, -0.17, 0.07), (0.05, 0.045, 0.05))):
        out = out + amp * torch.sin(fx * x + fy * y + ph[:, :, k].view(b, 3, 1, 1))
    return out


def _bump(b, h, w, cx, cy, rx, ry):
    y = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1) / max(h - 1, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w) / max(w - 1, 1)
    return torch.exp(-(((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2)).expand(b, 1, h, w)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 inputs of a loss case: tgt, refs, disp, K, inv_K, axisangle / translation [B,F,1,3], the invert flags, T (the fp64
    transformation_from_parameters of them rounded once) and the upstream map g (not yet masked)."""
    c = CASES[name]
    b, h, w, nf = c["B"], c["H"], c["W"], c["F"]
    tag = "reproj:" + name
    k, kinv = intrinsics(b, h, w)
    tgt = pattern(b, h, w, tag + ":tgt")
    refs = []
    for f in range(nf):
        ftag = tag + ":ref%d" % (0 if c.get("twins") else f)
        r = pattern(b, h, w, tag + ":tgt", c["shift"][f])
        if c.get("select"):
            # static content (the unshifted target: the identity term wins, the reprojection moves it away) in the upper part of the image,
            # moving content (the shifted copy the reprojection matches) in the lower part; frame f is clean in its own half and
            # carries a strong smooth perturbation in the other half, where the other frame then wins
            static = 1 / (1 + torch.exp((torch.arange(h, dtype=torch.float64).view(1, 1, h, 1) / (h - 1) - 0.42) * 14))
            r = static * tgt + (1 - static) * r
            r = r + 0.9 * (1 - _bump(b, h, w, 0.15 + 0.7 * f, 0.5, 0.42, 0.9)) * (pattern(b, h, w, ftag + ":q") - 0.5)
        r = r + c.get("pert", 0.04) * (pattern(b, h, w, ftag + ":p") - 0.5)
        refs.append(r.float())
    disp = 0.02 + 0.06 * (pattern(b, h, w, tag + ":disp")[:, :1] - 0.1) / 0.8
    if c.get("select"):
        disp = 0.024 + 0.15 * (disp - 0.05)                      # depths around the one the frames' translations are made for
    aa = detgen.uniform((b, nf, 1, 3), tag + ":aa", -c["rot"], c["rot"])
    tr = detgen.uniform((b, nf, 1, 3), tag + ":t", -c["trans"], c["trans"])
    if c.get("select"):
        # the translation that moves a point at the mid depth by the frame's shift
        depth_mid = 1 / (1 / MAX_DEPTH + (1 / MIN_DEPTH - 1 / MAX_DEPTH) * 0.024)
        for f in range(nf):
            sign = -1.0 if f % 2 else 1.0                      # (an inverted frame moves by -t)
            tr[:, f, 0, 0] = sign * c["shift"][f][0] * depth_mid / float(k[0, 0, 0])
            tr[:, f, 0, 1] = sign * c["shift"][f][1] * depth_mid / float(k[0, 1, 1])
            tr[:, f, 0, 2] = 0.0
    if "tz" in c:
        for f in range(nf):
            tr[:, f, 0, 2] = c["tz"][f]
    if c.get("twins"):
        aa[:, 1], tr[:, 1] = aa[:, 0], tr[:, 0]
    invert = tuple(bool(f % 2) for f in range(nf)) if not c.get("twins") else (False, False)
    T = [transformation_from_parameters(aa[:, f].double(), tr[:, f].double(), invert[f]).float() for f in range(nf)]
    return dict(tgt=tgt.float(), refs=refs, disp=disp.float(), K=k, inv_K=kinv, axisangle=aa, translation=tr, invert=invert, T=T,
                g=detgen.uniform((b, 1, h, w), tag + ":g", 0.2, 1.0))


# ------------------------------------------------------------------------------------------- the reference's layers, restated
def rot_from_axisangle(vec):
    """reference layers.py:64-103 ([B,1,3] -> [B,4,4]) in vec's dtype"""
    angle = torch.norm(vec, 2, 2, True)
    axis = vec / (angle + 1e-7)
    ca, sa = torch.cos(angle), torch.sin(angle)
    C = 1 - ca
    x, y, z = axis[..., 0].unsqueeze(1), axis[..., 1].unsqueeze(1), axis[..., 2].unsqueeze(1)
    xs, ys, zs, xC, yC, zC = x * sa, y * sa, z * sa, x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    rows = [[x * xC + ca, xyC - zs, zxC + ys], [xyC + zs, y * yC + ca, yzC - xs], [zxC - ys, yzC + xs, z * zC + ca]]
    r3 = torch.stack([torch.stack([e.reshape(-1) for e in row], 1) for row in rows], 1)                     # [B,3,3]
    return _homogeneous(r3, torch.zeros((vec.shape[0], 3, 1), dtype=vec.dtype))


def _homogeneous(r3, t):
    """[[r3, t], [0, 0, 0, 1]] as [B,4,4]"""
    bottom = torch.tensor([0, 0, 0, 1], dtype=r3.dtype).expand(r3.shape[0], 1, 4)
    return torch.cat([torch.cat([r3, t], 2), bottom], 1)


def get_translation_matrix(t):
    """reference layers.py:48-61"""
    b = t.shape[0]
    return _homogeneous(torch.eye(3, dtype=t.dtype).repeat(b, 1, 1), t.reshape(b, 3, 1))


def transformation_from_parameters(axisangle, translation, invert=False, mutant_order=False):
    """reference layers.py:28-45; mutant_order: T R computed where R^T T(-t) is asked for"""
    R = rot_from_axisangle(axisangle)
    t = translation
    if invert and not mutant_order:
        R, t = R.transpose(1, 2), -t
    T = get_translation_matrix(t)
    return torch.matmul(R, T) if (invert and not mutant_order) else torch.matmul(T, R)


def disp_to_depth(disp):
    return 1 / (1 / MAX_DEPTH + (1 / MIN_DEPTH - 1 / MAX_DEPTH) * disp)


def backproject(depth, inv_K):
    """reference layers.py:139-165 without its parameters: [B,1,H,W] -> [B,4,H*W]"""
    b, _, h, w = depth.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=depth.dtype), torch.arange(w, dtype=depth.dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, dtype=depth.dtype)], 0).unsqueeze(0).expand(b, 3, h * w)
    cam = depth.reshape(b, 1, -1) * torch.matmul(inv_K[:, :3, :3], pix)
    return torch.cat([cam, torch.ones((b, 1, h * w), dtype=depth.dtype)], 1)


def project(points, K, T, h, w, eps=1e-7, clamp_z=False, div_w=False):
    """reference layers.py:168-190: -> ([B,H,W,2] grid, c[2] [B,H,W]).  clamp_z / div_w: mutants"""
    b = points.shape[0]
    P = torch.matmul(K, T)[:, :3, :]
    cam = torch.matmul(P, points)
    z = cam[:, 2, :]
    zz = z.clamp(min=1e-3) if clamp_z else z
    pix = cam[:, :2, :] / (zz.unsqueeze(1) + eps)
    pix = pix.reshape(b, 2, h, w).permute(0, 2, 3, 1)
    px = pix[..., 0] / (w if div_w else w - 1)
    py = pix[..., 1] / (h - 1)
    return (torch.stack([px, py], -1) - 0.5) * 2, z.reshape(b, h, w)


def ssim_raw(x, y):
    """reference layers.py:215-245 before its clamp"""
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sig_x = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
    sig_y = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
    sig_xy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sig_xy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sig_x + sig_y + 0.03 ** 2)
    return (1 - n / d) / 2


def term(pred, tgt, w=SSIM_W):
    """[B,H,W]"""
    return w * torch.clamp(ssim_raw(pred, tgt), 0, 1).mean(1) + (1 - w) * (tgt - pred).abs().mean(1)


def unnormalise(vn, n, align):
    return (vn + 1) / 2 * (n - 1) if align else ((vn + 1) * n - 1) / 2


def evaluate(tgt, refs, disp, K, inv_K, T, align, automask, padding="border", tie_last=False, clamp_z=False, div_w=False):
    """The composition of the module docstring in the dtype of its inputs.  Returns a dict: m [B,1,H,W], loss, sel [B,1,H,W] (int64),
    terms [C,B,H,W] and per source frame pred, grid, z.  The keyword switches are the mutants of tests/test_reproj_audit_host.py."""
    b, _, h, w = tgt.shape
    points = backproject(disp_to_depth(disp), inv_K)
    preds, grids, zs, ident, reproj = [], [], [], [], []
    for r, t in zip(refs, T):
        grid, z = project(points, K, t, h, w, clamp_z=clamp_z, div_w=div_w)
        pred = F.grid_sample(r, grid, mode="bilinear", padding_mode=padding, align_corners=align)
        preds.append(pred); grids.append(grid); zs.append(z)
        reproj.append(term(pred, tgt))
        if automask:
            ident.append(term(r, tgt))
    terms = torch.stack(ident + reproj, 0)
    if tie_last:
        sel = terms.shape[0] - 1 - torch.flip(terms, (0,)).detach().min(0)[1]
    else:
        sel = torch.zeros(terms.shape[1:], dtype=torch.int64)
        best = terms[0].detach()
        for ch in range(1, terms.shape[0]):
            lower = terms[ch].detach() < best
            sel = torch.where(lower, torch.full_like(sel, ch), sel)
            best = torch.where(lower, terms[ch].detach(), best)
    m = terms.gather(0, sel.unsqueeze(0))[0].unsqueeze(1)
    return dict(m=m, loss=m.mean(), sel=sel.unsqueeze(1), terms=terms, pred=preds, grid=grids, z=zs)


# ------------------------------------------------------------------------------------------------------- the fragile pixels
def _dilate(mask):
    """bool [B,H,W] -> its 3x3 dilation"""
    return F.max_pool2d(mask.double().unsqueeze(1), 3, 1, 1)[:, 0] > 0


@functools.lru_cache(maxsize=None)
def fragile(name, align, automask, ties=True):
    """bool [B,1,H,W] from the fp64 evaluation of the case (module docstring); asserts the cap.  ties=False leaves the near-tie rule
    out (the twins case: its ties are exact, and what is compared is which of two equal channels takes the gradient)."""
    i = inputs(name)
    d = lambda t: t.double()
    tgt = d(i["tgt"])
    b, _, h, w = tgt.shape
    ev = evaluate(tgt, [d(r) for r in i["refs"]], d(i["disp"]), d(i["K"]), d(i["inv_K"]), [d(t) for t in i["T"]], align, automask)
    out = torch.zeros((b, h, w), dtype=torch.bool)
    if ties and ev["terms"].shape[0] > 1:
        two = torch.sort(ev["terms"], 0)[0][:2]
        out |= (two[1] - two[0]) < TAU_TIE
    for r, pred, grid in zip(i["refs"], ev["pred"], ev["grid"]):
        raw = ssim_raw(pred, tgt)
        out |= ((raw.abs() < TAU_SSIM) | ((raw - 1).abs() < TAU_SSIM)).any(1)
        ix, iy = unnormalise(grid[..., 0], w, align), unnormalise(grid[..., 1], h, align)
        near = lambda v, n: ((v - v.round()).abs() < TAU_PX) & (v > -TAU_PX) & (v < n - 1 + TAU_PX)      # (clipped coordinates far outside: no footprint change)
        kink = ((tgt - pred).abs() < TAU_L1).any(1)
        out |= _dilate(near(ix, w) | near(iy, h) | kink)
    share = float(out.double().mean())
    assert share <= CAP, "%s (align %s, automask %s): %.2f %% of the pixels are fragile, cap %.0f %%" % (name, align, automask, 100 * share, 100 * CAP)
    return out.unsqueeze(1)


# -------------------------------------------------------------------------------------------------------------- references
def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


@functools.lru_cache(maxsize=None)
def reference(name, align, automask, dtype, ties=True):
    """dict(m, loss, sel, ddisp, dT (list), keep [B,1,H,W], near_tie [B,1,H,W]) of the composition in `dtype` on the case's fp32 inputs;
    the gradients are those of (m * g * keep).sum()."""
    i = inputs(name)
    keep = ~fragile(name, align, automask, ties)
    c = lambda t: t.to(dtype)
    disp, T = _leaf(i["disp"], dtype), [_leaf(t, dtype) for t in i["T"]]
    ev = evaluate(c(i["tgt"]), [c(r) for r in i["refs"]], disp, c(i["K"]), c(i["inv_K"]), T, align, automask)
    (ev["m"] * (i["g"] * keep).to(dtype)).sum().backward()
    near_tie = torch.zeros_like(keep)
    if ev["terms"].shape[0] > 1:
        two = torch.sort(ev["terms"].detach().double(), 0)[0][:2]
        near_tie = ((two[1] - two[0]) < TAU_TIE).unsqueeze(1)
    return dict(m=ev["m"].detach(), loss=ev["loss"].detach(), sel=ev["sel"], ddisp=disp.grad, dT=[t.grad for t in T], keep=keep,
                near_tie=near_tie, z=[z.detach() for z in ev["z"]], grid=[g.detach() for g in ev["grid"]])


def upstream(name, align, automask, ties=True):
    """the upstream map of the reduction="none" form: g, zero on the fragile pixels"""
    return inputs(name)["g"] * (~fragile(name, align, automask, ties))


def win_shares(name, align, automask=True):
    """share of the pixels every channel wins, fp64"""
    sel = reference(name, align, automask, torch.float64)["sel"]
    nch = (2 if automask else 1) * CASES[name]["F"]
    return [float((sel == ch).double().mean()) for ch in range(nch)]


def motion_shares(name, align):
    """(share of sample coordinates outside the image, share of points with c[2] < 0) over the source frames, fp64"""
    r = reference(name, align, True, torch.float64)
    c = CASES[name]
    out, behind, n = 0, 0, 0
    for grid, z in zip(r["grid"], r["z"]):
        ix, iy = unnormalise(grid[..., 0], c["W"], align), unnormalise(grid[..., 1], c["H"], align)
        out += int(((ix < 0) | (ix > c["W"] - 1) | (iy < 0) | (iy > c["H"] - 1)).sum())
        behind += int((z < 0).sum())
        n += z.numel()
    return out / n, behind / n


# --------------------------------------------------------------------------------------------------- pose / geometry layers
def pose_vectors():
    """(axisangle, translation) [B,1,3]: angles up to 3 rad, plus the zero rotation as the last element"""
    b, a = POSE_CASE["B"], POSE_CASE["angle"]
    aa = detgen.uniform((b, 1, 3), "reproj:pose:aa", -a / 3 ** 0.5, a / 3 ** 0.5)
    aa[0] = torch.tensor([[a * 0.6, -a * 0.7, a * 0.35]])
    return aa, detgen.uniform((b, 1, 3), "reproj:pose:t", -1, 1)


def pose_weight():
    return detgen.uniform((POSE_CASE["B"], 4, 4), "reproj:pose:w", -1, 1)


@functools.lru_cache(maxsize=None)
def pose_reference(invert, dtype, mutant_order=False):
    """(M, daxisangle, dtranslation) of transformation_from_parameters under the fixed weight"""
    aa, tr = pose_vectors()
    a, t = _leaf(aa, dtype), _leaf(tr, dtype)
    m = transformation_from_parameters(a, t, invert, mutant_order)
    (m * pose_weight().to(dtype)).sum().backward()
    return m.detach(), a.grad, t.grad


def geom_inputs(size):
    h, w = size
    b, tag = 2, "reproj:geom:%dx%d" % size
    k, kinv = intrinsics(b, h, w)
    aa, tr = detgen.uniform((b, 1, 3), tag + ":aa", -0.2, 0.2), detgen.uniform((b, 1, 3), tag + ":t", -0.3, 0.3)
    return dict(depth=detgen.uniform((b, 1, h, w), tag + ":depth", 1.0, 20.0), K=k, inv_K=kinv,
                T=transformation_from_parameters(aa.double(), tr.double()).float(),
                gp=detgen.uniform((b, 4, h * w), tag + ":gp", -1, 1), gg=detgen.uniform((b, h, w, 2), tag + ":gg", -1, 1))


@functools.lru_cache(maxsize=None)
def geom_reference(size, dtype):
    """dict of BackprojectDepth (points, ddepth under gp) and Project3D on those points (grid, dpoints, dT under gg)"""
    i = geom_inputs(size)
    h, w = size
    depth = _leaf(i["depth"], dtype)
    pts = backproject(depth, i["inv_K"].to(dtype))
    (pts * i["gp"].to(dtype)).sum().backward()
    p, t = _leaf(pts.detach(), dtype), _leaf(i["T"], dtype)
    grid, _ = project(p, i["K"].to(dtype), t, h, w)
    (grid * i["gg"].to(dtype)).sum().backward()
    return dict(points=pts.detach(), ddepth=depth.grad, grid=grid.detach(), dpoints=p.grad, dT=t.grad)


# ------------------------------------------------------------------------------------------------------------------ PoseCNN
POSE_CNN_KEYS = ["net.%d.%s" % (i, p) for i in range(7) for p in ("weight", "bias")] + ["pose_conv.weight", "pose_conv.bias"]
POSE_CNN_SHAPE = (2, 6, 64, 96)


def pose_cnn_state(num_input_frames=2, tag="posecnn"):
    planes, kernels = (16, 32, 64, 128, 256, 256, 256), (7, 5, 3, 3, 3, 3, 3)
    sd, c_in = {}, 3 * num_input_frames
    for i, (c, k) in enumerate(zip(planes, kernels)):
        sd["net.%d.weight" % i], sd["net.%d.bias" % i] = torch.empty(c, c_in, k, k), torch.empty(c)
        c_in = c
    sd["pose_conv.weight"], sd["pose_conv.bias"] = torch.empty(6 * (num_input_frames - 1), c_in, 1, 1), torch.empty(6 * (num_input_frames - 1))
    return detgen.fill_state_dict(sd, tag)


def pose_cnn_forward(sd, x, num_input_frames=2):
    """reference networks/pose_cnn.py:36-50 as functional torch on a state_dict -> (axisangle, translation)"""
    out = x
    for i, k in enumerate((7, 5, 3, 3, 3, 3, 3)):
        out = F.relu(F.conv2d(out, sd["net.%d.weight" % i], sd["net.%d.bias" % i], 2, (k - 1) // 2))
    out = F.conv2d(out, sd["pose_conv.weight"], sd["pose_conv.bias"])
    out = 0.01 * out.mean(3).mean(2).view(-1, num_input_frames - 1, 1, 6)
    return out[..., :3], out[..., 3:]


def pose_cnn_input():
    b, c, h, w = POSE_CNN_SHAPE
    return torch.cat([detgen.image_batch(b, h, w, "posecnn:x%d" % i) for i in range(c // 3)], 1)


def pose_cnn_weights():
    b = POSE_CNN_SHAPE[0]
    return detgen.uniform((b, 1, 1, 3), "posecnn:ga", -1, 1), detgen.uniform((b, 1, 1, 3), "posecnn:gt", -1, 1)


@functools.lru_cache(maxsize=None)
def pose_cnn_reference(dtype):
    """(axisangle, translation, {key: gradient}) under the fixed output weights"""
    sd = {k: _leaf(v, dtype) for k, v in pose_cnn_state().items()}
    aa, tr = pose_cnn_forward(sd, pose_cnn_input().to(dtype))
    ga, gt = pose_cnn_weights()
    ((aa * ga.to(dtype)).sum() + (tr * gt.to(dtype)).sum()).backward()
    return aa.detach(), tr.detach(), {k: v.grad for k, v in sd.items()}
