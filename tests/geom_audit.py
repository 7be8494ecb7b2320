"""fp64 audit of the geometry / photometric / smoothness kernels (csrc/dn_warp.hip, the smooth2 part of csrc/dn_loss.hip): the
cases, the fragile-pixel rule and the measured tolerance (a plain module, importable without a GPU; the pattern of conv_audit.py).

CASES are closed-form inputs (oracle.detgen + pose literals) at the smallest shapes that still fire the branch they are named
for; tests/test_geom_audit_host.py asserts that they do (out-of-range share, Z < 1e-3 share, pixels per thread).  Without a mask
the photometric loss keeps its fragile pixels, and its loss and pose tolerances carry n_fragile x the largest per-pixel term
instead (photo_allowance); for the pose gradient that allowance is of the size of the gradient itself, so the pose comparison that
binds is the masked one.

fragile(): the warp is discontinuous in its coordinates -- a bilinear footprint changes at every integer ix / iy (the value is
continuous there, its gradient is not), the zeros substitution and the border clip switch at |xn| = 1 / at the first and last
pixel, the clamp gate at Z = 1e-3.  An fp32 evaluation may land on the other side of such a point than fp64 does, and both are
right.  Those pixels are found from the fp64 coordinates and REMOVED from the comparison before it is made (the upstream gradient
/ the explainability mask is zero there, so neither side's sums see them); a case may lose at most CAP of its pixels this way.

check(): the tolerance is measured, not preset.  Both the kernel and the fp32 oracle (torch on the CPU, `ref32`, evaluated by the
caller -- never the kernel) are fp32 evaluations of the same formula chain; they differ in operation order and FMA contraction.
So |got - ref64| <= MARGIN * max|ref32 - ref64| + FLOOR * max|ref64| over the kept elements, and the relative L2 error is held
to MARGIN times the fp32 oracle's own relative L2 error (+ FLOOR).  Every mutant of tests/test_geom_audit_host.py lands at least
10 x beyond that.

Measured on an MI355X: the worst err / max(max|ref32 - ref64|, FLOOR * max|ref64| / MARGIN) per quantity over all cases and
modes (tests/test_gpu_geom_fp64.py prints every figure) --
  inverse_warp (5 cases x 8 modes)   warped 1.41   ddepth 1.70   dpose 3.37 (oob_wide, quat, zeros: 64 block partials and a
                                     wave tree against torch's pairwise sum -- the largest figure of the audit)
  photo_3ref (8 modes)               loss 1.17   ddepth per scale 1.82   dpose (masked) 1.15   dmask 1.08
  big_angles                         pose_vec2mat 1.89   euler2mat 1.89   quat2mat 1.00   (their gradients 0.54 or less)
  ssim_min                           ssim 1.00   dx 1.53   dy 1.20;   ssim(x, x): exactly 0 at every size
  edge_min                           loss 1.25   ddisp 1.84
  smooth_min                         loss 3.11 (1x2x3x9: four fp32 quotients added, the oracle adds four fp32 means)   dmap 1.77
  smooth_min, plateau maps           gradient within 0.2 of sign_exact_tol(), itself 1e-5 of what one wrong sign would move it by
No quantity needs more than 3.4 of the margin of 16.

What the cases cannot reach: warp_pixel's `sane` guard.  With Z clamped at 1e-3 and finite inputs |ix| stays below about 1e6, far
from the 1e9 the guard tests for; only a non-finite coordinate gets there, and grid_sample defines no reference for that.
"""
import functools
import itertools

import torch

from oracle import detgen, geometry as OG, image_ops as OI, losses as OL

U = 2.0 ** -24                # unit round-off of fp32
MARGIN = 16.0                 # kernel error allowed = MARGIN x the fp32 oracle's own error against fp64
FLOOR = 4.0 * U               # x max|ref64|: where the fp32 oracle happens to be exact
TAU_PX = 1e-3                 # fragile: ix / iy this close to an integer (pixels), |xn| / |yn| this close to 1 (normalised units)
TAU_Z = 1e-4                  # fragile: Z this close to Z_MIN
Z_MIN = 1e-3                  # the reference's clamp of the projected depth (inverse_warp.py:62)
CAP = 0.02                    # a case may leave out at most this share of its pixels
WARP_THREADS = 64 * 256       # dn_warp_blocks() caps the grid at 64 blocks of 256 threads

ROTS = ("euler", "quat")
PADS = ("zeros", "border")
ALIGNS = (False, True)
WARP_MODES = tuple(itertools.product(ROTS, PADS, ALIGNS))
PHOTO_MODES = tuple((rot, pad, ac, m) for (rot, pad) in (("euler", "zeros"), ("quat", "border")) for ac in ALIGNS for m in (False, True))

MIN_SIZES = ((2, 2), (2, 7), (3, 3), (5, 2), (4, 9))

CASES = {
    # zeros substitution (xdead / ydead) and border clip with its zeroed multiplier, ragged plane (851 pixels: 4 blocks, the last partial)
    "oob_ragged": dict(kind="warp", B=3, h=23, w=37, trans=0.6, rot=0.25, depth=(0.4, 20.0)),
    # most of the plane out of range, W not a multiple of the wavefront
    "oob_wide": dict(kind="warp", B=2, h=17, w=70, trans=1.0, rot=0.4, depth=(0.3, 8.0)),
    # Z < 1e-3 on more than a third of the pixels: coordinates of 1e3 .. 1e5 pixels, the clamp gate on dZ (it decides a gradient under border
    # padding, where a pixel clipped in x is often still inside in y; under zeros padding these pixels are already dead)
    "behind_camera": dict(kind="warp", B=3, h=23, w=37, depth=(0.3, 3.0),
                          pose=[[0.1, -0.05, -1.2, 0.03, -0.02, 0.04], [0.0, 0.0, -0.8, 0.0, 0.0, 0.0], [-0.2, 0.1, -2.0, 0.1, 0.1, -0.1]]),
    # Z < 1e-3 on pixels that still sample INSIDE the image (depths below the clamp under a near-identity pose: ix = j * Z / 1e-3), so that
    # the gate decides a gradient in every mode, zeros padding included
    "behind_live": dict(kind="warp", B=2, h=23, w=37, trans=1e-4, rot=0.05, depth=(2e-3, 2e-2), depth_low=(1e-4, 7e-4)),
    # 16 704 pixels > 64 * 256: the grid-stride loop takes a second pixel per thread, pose_proj_bwd sums 64 block partials
    "grid_stride": dict(kind="warp", B=1, h=72, w=232, trans=0.3, rot=0.1, depth=(1.0, 20.0)),
    "big_angles": dict(kind="pose", B=5, angle=3.0),
    # pose stride 6 * n_ref, accumulate_depth for reference i > 0, first_pose accumulation over the scales
    "photo_3ref": dict(kind="photo", B=2, h=24, w=40, scales=4, n_ref=3, trans=0.5, rot=0.2, depth=(0.4, 20.0)),
    "ssim_min": dict(kind="ssim", sizes=MIN_SIZES, planes=((1, 1), (2, 3))),
    "edge_min": dict(kind="edge", sizes=MIN_SIZES, planes=((2, 3), (2, 1))),
    "smooth_min": dict(kind="smooth", shapes=((2, 1, 3, 3), (1, 2, 3, 9), (2, 1, 7, 3), (3, 1, 17, 29))),
}
WARP_CASES = tuple(k for k, v in CASES.items() if v["kind"] == "warp")


# ------------------------------------------------------------------------------------------------------------------ inputs
def intrinsics(b, h, w):
    """KITTI's intrinsics scaled to h x w (fp32) and their inverse (inverted in fp64, rounded once)."""
    fx, fy, cx, cy = 241.67 * w / 416, 246.28 * h / 128, 204.17 * w / 416, 59.0 * h / 128
    k = torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float32).repeat(b, 1, 1)
    return k, torch.inverse(k.double()).float()


def _poses(shape, tag, trans, rot):
    return torch.cat([detgen.uniform(shape + (3,), tag + ":t", -trans, trans), detgen.uniform(shape + (3,), tag + ":r", -rot, rot)], -1)


@functools.lru_cache(maxsize=None)
def warp_inputs(name):
    """fp32 inputs of a warp case: img, depth, pose, K, Kinv and the upstream gradient gw (not yet masked)."""
    c = CASES[name]
    b, h, w = c["B"], c["h"], c["w"]
    tag = "geom:" + name
    k, kinv = intrinsics(b, h, w)
    pose = torch.tensor(c["pose"], dtype=torch.float32) if "pose" in c else _poses((b,), tag + ":pose", c["trans"], c["rot"])
    depth = detgen.uniform((b, h, w), tag + ":depth", *c["depth"])
    if "depth_low" in c:                                   # half of the pixels below the clamp, none near it
        depth = torch.where(detgen.bernoulli((b, h, w), tag + ":low", 0.5), detgen.uniform((b, h, w), tag + ":depth_low", *c["depth_low"]), depth)
    return dict(img=detgen.uniform((b, 3, h, w), tag + ":img", -1, 1), depth=depth,
                pose=pose, K=k, Kinv=kinv, gw=detgen.uniform((b, 3, h, w), tag + ":g", -1, 1))


@functools.lru_cache(maxsize=None)
def photo_inputs(name):
    c = CASES[name]
    b, h, w, tag = c["B"], c["h"], c["w"], "geom:" + name
    k, kinv = intrinsics(b, h, w)
    sizes = [(h >> i, w >> i) for i in range(c["scales"])]
    return dict(tgt=detgen.uniform((b, 3, h, w), tag + ":tgt", -1, 1),
                refs=[detgen.uniform((b, 3, h, w), tag + ":ref%d" % i, -1, 1) for i in range(c["n_ref"])],
                depth=[detgen.uniform((b, 1, hh, ww), tag + ":d%d" % i, *c["depth"]) for i, (hh, ww) in enumerate(sizes)],
                mask=[detgen.uniform((b, c["n_ref"], hh, ww), tag + ":m%d" % i, 0.1, 0.9) for i, (hh, ww) in enumerate(sizes)],
                pose=_poses((b, c["n_ref"]), tag + ":pose", c["trans"], c["rot"]), K=k, Kinv=kinv, sizes=sizes)


def plateau(shape, tag):
    """floor(4 u) / 4: exact in fp32, first and second differences exact in both precisions, with many exact ties."""
    return torch.floor(4 * detgen.uniform(shape, tag)) / 4


# ---------------------------------------------------------------------------------------------------- fp64 coordinates
def project(depth, pose, K, Kinv, rot):
    """oracle.geometry.pixel2cam + the projection of cam2pixel restated: (X, Y, Z), each [B, h*w], in depth's dtype.  `pose` is
    [B, 6], or [B, h*w, 6] with one pose per pixel (a leaf whose gradient is then every pixel's own term of d pose)."""
    b, h, w = depth.shape
    dt = depth.dtype
    ii = torch.arange(h, dtype=dt).view(h, 1).expand(h, w)
    jj = torch.arange(w, dtype=dt).view(1, w).expand(h, w)
    pix = torch.stack((jj, ii, torch.ones_like(ii)), 0).reshape(1, 3, -1)
    cam = (Kinv @ pix) * depth.reshape(b, 1, -1)
    if pose.dim() == 2:
        proj = K @ OG.pose_vec2mat(pose, rot)
        pc = proj[:, :, :3] @ cam + proj[:, :, 3:]
    else:
        proj = K[:, None] @ OG.pose_vec2mat(pose.reshape(-1, 6), rot).reshape(b, h * w, 3, 4)
        pc = ((proj[..., :3] @ cam.permute(0, 2, 1)[..., None])[..., 0] + proj[..., 3]).permute(0, 2, 1)
    return pc[:, 0], pc[:, 1], pc[:, 2]


def normalise(X, Y, Z, h, w):
    zc = Z.clamp(min=Z_MIN)
    return 2 * (X / zc) / (w - 1) - 1, 2 * (Y / zc) / (h - 1) - 1


def unnormalise(vn, n, align):
    """grid_sample's map of a normalised coordinate to pixels"""
    return (vn + 1) / 2 * (n - 1) if align else ((vn + 1) * n - 1) / 2


def coords64(depth, pose, K, Kinv, rot, align):
    """Z, xn, yn (before the zeros substitution), ix, iy (before the border clip) in fp64, each [B, h, w]"""
    b, h, w = depth.shape
    X, Y, Z = project(depth.double(), pose.double(), K.double(), Kinv.double(), rot)
    xn, yn = normalise(X, Y, Z, h, w)
    return tuple(t.reshape(b, h, w) for t in (Z, xn, yn, unnormalise(xn, w, align), unnormalise(yn, h, align)))


def fragile_mask(depth, pose, K, Kinv, rot, align):
    """bool [B, h, w]: pixels where fp32 and fp64 may legitimately land on different sides of a discontinuity"""
    Z, xn, yn, ix, iy = coords64(depth, pose, K, Kinv, rot, align)
    near_int = lambda v: (v - v.round()).abs() < TAU_PX
    near_one = lambda v: (v.abs() - 1).abs() < TAU_PX
    return near_int(ix) | near_int(iy) | near_one(xn) | near_one(yn) | ((Z - Z_MIN).abs() < TAU_Z)


def _scaled_intrinsics(K, Kinv, down):
    return torch.cat((K[:, 0:2] / down, K[:, 2:]), dim=1), torch.cat((Kinv[:, :, 0:2] * down, Kinv[:, :, 2:]), dim=2)


@functools.lru_cache(maxsize=None)
def fragile(name, rot, align):
    """The fragile pixels of a case: bool [B, h, w] for a warp case, a list over the scales of bool [B, n_ref, h, w] for the
    photometric case.  Asserts the cap: a case that exceeds it gets another tag or pose, never another cap."""
    c = CASES[name]
    if c["kind"] == "warp":
        i = warp_inputs(name)
        out = fragile_mask(i["depth"], i["pose"], i["K"], i["Kinv"], rot, align)
        share = float(out.double().mean())
    else:
        i = photo_inputs(name)
        out = []
        for d in i["depth"]:
            ks, kinvs = _scaled_intrinsics(i["K"].double(), i["Kinv"].double(), c["h"] / d.shape[2])
            out.append(torch.stack([fragile_mask(d[:, 0], i["pose"][:, r], ks, kinvs, rot, align) for r in range(c["n_ref"])], 1))
        share = sum(int(f.sum()) for f in out) / sum(f.numel() for f in out)
    assert share <= CAP, "%s (%s, align %s): %.2f %% of the pixels are fragile, cap %.0f %%" % (name, rot, align, 100 * share, 100 * CAP)
    return out


def shares(name, rot):
    """(share of x coordinates out of [-1, 1], of y coordinates, of either, of Z < 1e-3, of Z < 1e-3 and inside, pixels per sample)
    in fp64"""
    i = warp_inputs(name)
    Z, xn, yn, _, _ = coords64(i["depth"], i["pose"], i["K"], i["Kinv"], rot, False)
    ox, oy = xn.abs() > 1, yn.abs() > 1
    f = lambda m: float(m.double().mean())
    return f(ox), f(oy), f(ox | oy), f(Z < Z_MIN), f((Z < Z_MIN) & ~ox & ~oy), Z.shape[1] * Z.shape[2]


# ------------------------------------------------------------------------------------------------------------ the checker
class Result(object):
    def __init__(self, name, ratio, excess, err, tol, rel, rel_tol):
        self.name, self.ratio, self.excess, self.err, self.tol, self.rel, self.rel_tol = name, ratio, excess, err, tol, rel, rel_tol

    def __str__(self):
        return "%-44s err %.3e tol %.3e | rel L2 %.3e tol %.3e | err / oracle32 %.2f | worst / tol %.3g" % (
            self.name, self.err, self.tol, self.rel, self.rel_tol, self.ratio, self.excess)


def compare(name, got, ref64, ref32, keep=None, extra=0.0):
    """`got` against `ref64` with the tolerance the fp32 oracle `ref32` measures (module docstring); `keep` (bool, broadcastable)
    selects the compared elements, `extra` is an explicit absolute allowance per element.  Returns a Result; never raises for a
    miss.  Result.ratio = max err / max(max|ref32 - ref64|, FLOOR * max|ref64| / MARGIN); Result.excess > 1 is a miss."""
    got, ref64, ref32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, "%s: shapes %s / %s / %s" % (name, tuple(got.shape), tuple(ref64.shape), tuple(ref32.shape))
    assert ref64.dtype == torch.float64
    if keep is not None:
        k = keep.expand_as(ref64)
        got, ref64, ref32 = got[k], ref64[k], ref32[k]
    got, ref64, ref32 = got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)
    assert ref64.numel() > 0, name
    scale = float(ref64.abs().max())
    base = float((ref32 - ref64).abs().max())
    tol = MARGIN * base + FLOOR * scale + extra
    err = float((got - ref64).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
    norm = float(ref64.norm()) + 1e-300
    rel_tol = MARGIN * float((ref32 - ref64).norm()) / norm + FLOOR + extra * ref64.numel() ** 0.5 / norm
    rel = float((got - ref64).norm()) / norm if err != float("inf") else float("inf")
    ratio = max(err - extra, 0.0) / max(base, FLOOR * scale / MARGIN, 1e-300)
    return Result(name, ratio, max(err / max(tol, 1e-300), rel / rel_tol), err, tol, rel, rel_tol)


def check(name, got, ref64, ref32, keep=None, extra=0.0, verbose=True):
    r = compare(name, got, ref64, ref32, keep, extra)
    if verbose:
        print("geom_audit " + str(r))
    assert r.excess <= 1.0, "outside the measured tolerance: " + str(r)
    return r


def sign_exact_tol(shape, weight=1.0):
    """smooth2's gradient on a map whose second differences are exact is (a0 / n0 + a3 / n3 + a12 / n1) * weight with integer sign
    sums |a0|, |a3| <= 4, |a12| <= 8: fp32 rounds three quotients, two sums and one product (<= 6 roundings of values below the sum
    of the largest terms), while ONE wrong sign moves it by at least weight / max(n) -- some 2^20 times more.  'Exactly the fp64
    gradient' therefore means: within this rounding allowance, and no measured margin."""
    b, c, h, w = shape
    n0, n1, n3 = b * c * h * (w - 2), b * c * (h - 1) * (w - 1), b * c * (h - 2) * w
    return 6 * U * (4.0 / n0 + 8.0 / n1 + 4.0 / n3) * weight


# ----------------------------------------------------------------------------------------------------------- references
def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


@functools.lru_cache(maxsize=None)
def warp_reference(name, rot, pad, align, dtype):
    """(warped, ddepth, dpose, keep) of oracle.geometry.inverse_warp in `dtype` on the case's fp32 inputs, the upstream gradient
    zeroed on the fragile pixels; keep = ~fragile as [B, 1, h, w]."""
    i = warp_inputs(name)
    keep = ~fragile(name, rot, align)[:, None]
    d, p = _leaf(i["depth"], dtype), _leaf(i["pose"], dtype)
    out = OG.inverse_warp(i["img"].to(dtype), d, p, i["K"].to(dtype), i["Kinv"].to(dtype), rot, pad, align)
    (out * (i["gw"] * keep).to(dtype)).sum().backward()
    return out.detach(), d.grad, p.grad, keep


def photo_masks(name, rot, align):
    """the case's explainability masks, zero on the fragile pixels"""
    return [m * (~f).to(m.dtype) for m, f in zip(photo_inputs(name)["mask"], fragile(name, rot, align))]


@functools.lru_cache(maxsize=None)
def photo_reference(name, rot, pad, align, with_mask, dtype):
    """(loss, [ddepth per scale], dpose [B, n_ref, 6], [dmask per scale] or None) of oracle.losses.photometric_reconstruction_loss"""
    i = photo_inputs(name)
    c = lambda t: t.to(dtype)
    depth = [_leaf(d, dtype) for d in i["depth"]]
    pose = _leaf(i["pose"], dtype)
    masks = [_leaf(m, dtype) for m in photo_masks(name, rot, align)] if with_mask else [None] * len(depth)
    v = OL.photometric_reconstruction_loss(c(i["tgt"]), [c(r) for r in i["refs"]], c(i["K"]), c(i["Kinv"]), depth, masks, pose, rot, pad, align)
    v.backward()
    return v.detach(), [d.grad for d in depth], pose.grad, [m.grad for m in masks] if with_mask else None


@functools.lru_cache(maxsize=None)
def photo_allowance(name, rot, pad, align):
    """Without an explainability mask the fragile pixels stay in the sums.  Returns (loss allowance, pose allowance [n_ref, 6],
    [keep per scale, bool [B, 1, h, w]]): n_fragile x the largest per-pixel term in fp64, per scale and reference, where a pixel's
    term of the loss is its sum over the channels of |diff| / count and its term of d pose is the gradient of a pose of its own."""
    c, i = CASES[name], photo_inputs(name)
    frag = fragile(name, rot, align)
    K, Kinv = i["K"].double(), i["Kinv"].double()
    loss_allow, pose_allow, keeps = 0.0, torch.zeros(c["n_ref"], 6, dtype=torch.float64), []
    for d, f in zip(i["depth"], frag):
        b, _, h, w = d.shape
        ks, kinvs = _scaled_intrinsics(K, Kinv, c["h"] / h)
        tgt_s = torch.nn.functional.interpolate(i["tgt"].double(), (h, w), mode="area")
        keeps.append(~f.any(1, keepdim=True))
        for r in range(c["n_ref"]):
            n = int(f[:, r].sum())
            if n == 0:
                continue
            ref_s = torch.nn.functional.interpolate(i["refs"][r].double(), (h, w), mode="area")
            pp = i["pose"][:, r].double()[:, None].expand(b, h * w, 6).clone().requires_grad_(True)
            X, Y, Z = project(d[:, 0].double(), pp, ks, kinvs, rot)
            xn, yn = normalise(X, Y, Z, h, w)
            if pad == "zeros":
                xn = torch.where(xn.detach().abs() > 1, torch.full_like(xn, 2.0), xn)
                yn = torch.where(yn.detach().abs() > 1, torch.full_like(yn, 2.0), yn)
            warped = torch.nn.functional.grid_sample(ref_s, torch.stack([xn, yn], 2).reshape(b, h, w, 2), padding_mode=pad, align_corners=align)
            oob = 1 - (warped == 0).prod(1, keepdim=True).type_as(warped)
            term = ((tgt_s - warped) * oob).abs().sum(1) / (b * 3 * h * w)          # [B, h, w]
            term.sum().backward()
            loss_allow += n * float(term.detach().max())
            pose_allow[r] += n * pp.grad.abs().amax(dim=(0, 1))
    return loss_allow, pose_allow, keeps


@functools.lru_cache(maxsize=None)
def pose_reference(rot, dtype):
    """big_angles: pose_vec2mat / euler2mat or quat2mat forward, and backward under a fixed weight: (mat, dvec, rmat, dangle)"""
    c = CASES["big_angles"]
    vec = detgen.uniform((c["B"], 6), "geom:big_angles", -c["angle"], c["angle"])
    wt = pose_weight()
    v = _leaf(vec, dtype)
    m = OG.pose_vec2mat(v, rot)
    (m * wt.to(dtype)).sum().backward()
    a = _leaf(vec[:, 3:], dtype)
    r = (OG.euler2mat if rot == "euler" else OG.quat2mat)(a)
    (r * wt[:, :, :3].to(dtype)).sum().backward()
    return m.detach(), v.grad, r.detach(), a.grad


def pose_vectors():
    c = CASES["big_angles"]
    return detgen.uniform((c["B"], 6), "geom:big_angles", -c["angle"], c["angle"])


def pose_weight():
    return detgen.uniform((CASES["big_angles"]["B"], 3, 4), "geom:big_angles:w", -1, 1)


def ssim_inputs(planes, size, same=False):
    shape = tuple(planes) + tuple(size)
    tag = "geom:ssim:%dx%dx%dx%d" % shape
    x = detgen.uniform(shape, tag + ":x")
    return x, (x.clone() if same else detgen.uniform(shape, tag + ":y")), detgen.uniform(shape, tag + ":g", -1, 1)


@functools.lru_cache(maxsize=None)
def ssim_reference(planes, size, dtype):
    x, y, g = ssim_inputs(planes, size)
    xl, yl = _leaf(x, dtype), _leaf(y, dtype)
    s = OI.ssim(xl, yl)
    (s * g.to(dtype)).sum().backward()
    return s.detach(), xl.grad, yl.grad


def edge_inputs(planes, size, flat=False):
    (b, c), (h, w) = planes, size
    tag = "geom:edge:%dx%dx%dx%d" % (b, c, h, w)
    disp = plateau((b, 1, h, w), tag + ":p") * 4 + 0.25 if flat else detgen.uniform((b, 1, h, w), tag + ":disp", 0.1, 5)
    return disp, detgen.uniform((b, c, h, w), tag + ":img")


@functools.lru_cache(maxsize=None)
def edge_reference(planes, size, flat, dtype):
    disp, img = edge_inputs(planes, size, flat)
    d = _leaf(disp, dtype)
    v = OI.get_smooth_loss(d, img.to(dtype))
    v.backward()
    return v.detach(), d.grad


def smooth_inputs(shape, flat):
    tag = "geom:smooth:%dx%dx%dx%d" % tuple(shape)
    return plateau(shape, tag + ":p") if flat else detgen.uniform(shape, tag + ":u", 0.1, 5)


@functools.lru_cache(maxsize=None)
def smooth_reference(shape, flat, dtype):
    m = _leaf(smooth_inputs(shape, flat), dtype)
    v = OL.smooth_loss(m)
    v.backward()
    return v.detach(), m.grad
