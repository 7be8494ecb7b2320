"""Host checks of tests/geom_audit.py, the fp64 audit of the warp / photometric / smoothness kernels (no GPU needed).

  * every case stays within the fragile-pixel cap and fires the branch it is named for by a stated share;
  * the fp32 oracle passes check() against the fp64 oracle (it is `ref32`), and so does this file's own restatement of the warp
    (projection, substitution, clip, bilinear taps written out) that the mutants are built from;
  * the checker rejects what it is for: ten fp64 mutants of the oracle, each at least 10 x beyond the tolerance on the case named.
    This is the evidence that tests/test_gpu_geom_fp64.py would fail on a kernel that is wrong in that way.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import geom_audit as GA  # noqa: E402
from oracle import geometry as OG, image_ops as OI, losses as OL  # noqa: E402

F64, F32 = torch.float64, torch.float32
REJECT = 10.0               # a mutant must land at least this far beyond the tolerance


# ------------------------------------------------------------------------------------------ cases: caps and branch shares
@pytest.mark.parametrize("name", GA.WARP_CASES + ("photo_3ref",))
def test_fragile_share_within_cap(name):
    for rot in GA.ROTS:
        for ac in GA.ALIGNS:
            f = GA.fragile(name, rot, ac)                      # asserts the cap itself
            fl = f if isinstance(f, list) else [f]
            share = sum(int(x.sum()) for x in fl) / sum(x.numel() for x in fl)
            print("%s %s align %d: %.2f %% fragile" % (name, rot, ac, 100 * share))
            assert share <= GA.CAP


def test_fragile_cap_is_enforced():
    """a tau that flags a tenth of the plane trips the assertion inside fragile() (the cap is code, not prose)"""
    tau = GA.TAU_PX
    GA.fragile.cache_clear()
    try:
        GA.TAU_PX = 0.05
        with pytest.raises(AssertionError, match="fragile"):
            GA.fragile("oob_ragged", "euler", False)
    finally:
        GA.TAU_PX = tau
        GA.fragile.cache_clear()


def test_cases_fire_their_branches():
    for name in GA.WARP_CASES:
        for rot in GA.ROTS:
            ox, oy, either, behind, behind_inside, pixels = GA.shares(name, rot)
            print("%-14s %-5s out of range x %.1f %% y %.1f %% either %.1f %% | Z < 1e-3 %.1f %%, and inside %.1f %% | %d pixels" % (
                name, rot, 100 * ox, 100 * oy, 100 * either, 100 * behind, 100 * behind_inside, pixels))
            if name != "behind_live":
                assert either >= 0.10, (name, rot)
            else:
                assert behind_inside >= 0.25, (name, rot)
            if name in ("oob_ragged", "oob_wide"):
                assert ox >= 0.10 and oy >= 0.10, (name, rot)
            if name == "oob_wide":
                assert either >= 0.50, (name, rot)
            if name == "behind_camera":
                assert behind >= 0.25, (name, rot)
            if name == "grid_stride":
                assert pixels > GA.WARP_THREADS
    c = GA.CASES["photo_3ref"]
    assert c["n_ref"] == 3 and GA.photo_inputs("photo_3ref")["sizes"] == [(24, 40), (12, 20), (6, 10), (3, 5)]
    assert abs(float(GA.pose_vectors()[:, 3:].abs().max())) > 2.5          # big_angles really leaves today's +-0.7


# ------------------------------------------------------------------------------------- the fp32 oracle passes trivially
def test_fp32_oracle_passes():
    for name in GA.WARP_CASES:
        for mode in GA.WARP_MODES:
            r64, r32 = GA.warp_reference(name, *mode, F64), GA.warp_reference(name, *mode, F32)
            tag = "%s:%s:%s:ac%d" % ((name,) + mode)
            GA.check(tag + ":warped", r32[0], r64[0], r32[0], keep=r64[3], verbose=False)
            GA.check(tag + ":ddepth", r32[1], r64[1], r32[1], verbose=False)
            GA.check(tag + ":dpose", r32[2], r64[2], r32[2], verbose=False)
    for mode in GA.PHOTO_MODES:
        r64, r32 = GA.photo_reference("photo_3ref", *mode, F64), GA.photo_reference("photo_3ref", *mode, F32)
        GA.check("photo:loss", r32[0], r64[0], r32[0], verbose=False)
        GA.check("photo:dpose", r32[2], r64[2], r32[2], verbose=False)


# ------------------------------------------------------------------------------------------------------- the warp, restated
def bilinear(img, ix, iy):
    """4-tap bilinear gather of img [B, C, h, w] at (ix, iy) [B, P], taps outside the image are 0; differentiable in ix, iy"""
    b, c, h, w = img.shape
    x0, y0 = ix.detach().floor(), iy.detach().floor()
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = 1 - wx1, 1 - wy1
    flat = img.reshape(b, c, h * w)

    def tap(xx, yy):
        inb = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).long()
        return flat.gather(2, idx[:, None].expand(b, c, idx.shape[1])) * inb[:, None].to(img.dtype)

    out = (tap(x0, y0) * (wx0 * wy0)[:, None] + tap(x0 + 1, y0) * (wx1 * wy0)[:, None]
           + tap(x0, y0 + 1) * (wx0 * wy1)[:, None] + tap(x0 + 1, y0 + 1) * (wx1 * wy1)[:, None])
    return out.reshape(b, c, h, w)


def _straight_through(clipped, raw):
    """the clipped value with the gradient of the raw one"""
    return raw + (clipped - raw).detach()


def warp_variant(img, depth, pose, K, Kinv, rot, pad, align, substitute=True, z_pass=False, clip_pass=False):
    """oracle.geometry.inverse_warp written out, with the switches the mutants flip"""
    b, h, w = depth.shape
    X, Y, Z = GA.project(depth, pose, K, Kinv, rot)
    zc = Z.clamp(min=GA.Z_MIN)
    if z_pass:
        zc = _straight_through(zc, Z)
    xn, yn = 2 * (X / zc) / (w - 1) - 1, 2 * (Y / zc) / (h - 1) - 1
    if pad == "zeros" and substitute:
        xn = torch.where(xn.detach().abs() > 1, torch.full_like(xn, 2.0), xn)
        yn = torch.where(yn.detach().abs() > 1, torch.full_like(yn, 2.0), yn)
    ix, iy = GA.unnormalise(xn, w, align), GA.unnormalise(yn, h, align)
    if pad == "border":
        cx, cy = ix.clamp(0, w - 1), iy.clamp(0, h - 1)
        ix, iy = (_straight_through(cx, ix), _straight_through(cy, iy)) if clip_pass else (cx, cy)
    return bilinear(img, ix, iy)


def run_warp(name, rot, align, fn, per_pixel_pose=False):
    """(warped, ddepth, dpose) in fp64 of fn(img, depth, pose, K, Kinv) on the case's inputs, with the upstream gradient the audit
    uses (zero on the pixels fragile for the TRUE mode); with per_pixel_pose, dpose is [B, h*w, 6]: every pixel's own term"""
    i = GA.warp_inputs(name)
    keep = ~GA.fragile(name, rot, align)[:, None]
    d, p = GA._leaf(i["depth"], F64), GA._leaf(i["pose"], F64)
    if per_pixel_pose:
        p = i["pose"].double()[:, None].expand(-1, d.shape[1] * d.shape[2], 6).clone().requires_grad_(True)
    out = fn(i["img"].double(), d, p, i["K"].double(), i["Kinv"].double())
    (out * (i["gw"] * keep).double()).sum().backward()
    return out.detach(), d.grad, p.grad


def excess(name, mode, got, quantities=("warped", "ddepth", "dpose")):
    """how far beyond the tolerance `got` (warped, ddepth, dpose) lands on the case in its TRUE mode: {quantity: excess}"""
    r64, r32 = GA.warp_reference(name, *mode, F64), GA.warp_reference(name, *mode, F32)
    out = {}
    for q, k in (("warped", 0), ("ddepth", 1), ("dpose", 2)):
        if q in quantities:
            out[q] = GA.compare("%s:%s" % (name, q), got[k], r64[k], r32[k], keep=r64[3] if k == 0 else None).excess
    return out


def test_restated_warp_passes():
    """the restatement the mutants are built from is the oracle: every case and mode passes check() unmutated"""
    for name in GA.WARP_CASES:
        for mode in GA.WARP_MODES:
            rot, pad, ac = mode
            got = run_warp(name, rot, ac, lambda *a: warp_variant(*a, rot, pad, ac))
            for q, e in excess(name, mode, got).items():
                assert e <= 1.0, (name, mode, q, e)
    name, (rot, pad, ac) = "grid_stride", GA.WARP_MODES[0]
    per_pixel = run_warp(name, rot, ac, lambda *a: warp_variant(*a, rot, pad, ac), per_pixel_pose=True)[2]
    e = excess(name, (rot, pad, ac), (None, None, per_pixel.sum(1)), ("dpose",))
    assert e["dpose"] <= 1.0, e                                   # the per-pixel pose terms sum to the oracle's d pose


# ------------------------------------------------------------------------------------------------------------- the mutants
def _report(n, what, ex):
    print("mutant %2d %-58s %s" % (n, what, "  ".join("%s %.3g x" % kv for kv in sorted(ex.items()))))


def test_mutant_01_padding_mode_swapped():
    for rot, pad, ac in GA.WARP_MODES:
        other = "border" if pad == "zeros" else "zeros"
        got = run_warp("oob_ragged", rot, ac, lambda *a: OG.inverse_warp(*a, rot, other, ac))
        ex = excess("oob_ragged", (rot, pad, ac), got)
        _report(1, "padding %s computed as %s (%s, align %d)" % (pad, other, rot, ac), ex)
        assert min(ex.values()) >= REJECT


def test_mutant_02_align_corners_swapped():
    for rot, pad, ac in GA.WARP_MODES:
        got = run_warp("oob_ragged", rot, ac, lambda *a: OG.inverse_warp(*a, rot, pad, not ac))
        ex = excess("oob_ragged", (rot, pad, ac), got)
        _report(2, "align_corners %d computed as %d (%s, %s)" % (ac, not ac, rot, pad), ex)
        assert min(ex.values()) >= REJECT


def test_mutant_03_zeros_without_substitution():
    for rot in GA.ROTS:
        got = run_warp("oob_wide", rot, False, lambda *a: warp_variant(*a, rot, "zeros", False, substitute=False))
        ex = excess("oob_wide", (rot, "zeros", False), got, ("warped",))
        _report(3, "zeros padding without the := 2 substitution (%s, align 0)" % rot, ex)
        assert ex["warped"] >= REJECT


def test_mutant_04_z_clamp_passes_gradient():
    """The gate decides a gradient only where a pixel with Z < 1e-3 still has a live coordinate.  On behind_camera every clamped pixel
    lands 1e3 .. 1e5 pixels outside in x or y: under zeros padding the substitution has then emptied all four taps and the mutant is
    invisible (printed: ~1e-11 of the tolerance, fp64 noise); under border padding the other coordinate is often still inside and the
    gate is what removes its dZ term.  behind_live keeps the clamped pixels inside the image, so every mode sees the gate."""
    for rot, pad, ac in GA.WARP_MODES:
        for name in ("behind_camera", "behind_live"):
            got = run_warp(name, rot, ac, lambda *a: warp_variant(*a, rot, pad, ac, z_pass=True))
            ex = excess(name, (rot, pad, ac), got, ("ddepth", "dpose"))
            _report(4, "Z clamp passes gradient below 1e-3 (%s: %s, %s, align %d)" % (name, rot, pad, ac), ex)
            assert min(ex.values()) >= REJECT or (name == "behind_camera" and pad == "zeros")


def test_mutant_05_border_clip_passes_gradient():
    for name in ("oob_ragged", "oob_wide"):
        for rot in GA.ROTS:
            for ac in GA.ALIGNS:
                got = run_warp(name, rot, ac, lambda *a: warp_variant(*a, rot, "border", ac, clip_pass=True))
                ex = excess(name, (rot, "border", ac), got, ("ddepth", "dpose"))
                _report(5, "border clip passes gradient on clipped coordinates (%s, %s, align %d)" % (name, rot, ac), ex)
                assert min(ex.values()) >= REJECT


def test_mutant_06_pose_gradient_without_the_last_block():
    for rot, pad, ac in GA.WARP_MODES:
        per_pixel = run_warp("grid_stride", rot, ac, lambda *a: warp_variant(*a, rot, pad, ac), per_pixel_pose=True)[2]
        dropped = per_pixel[:, :-256].sum(1).clone()
        dropped[:-1] = per_pixel[:-1].sum(1)                      # only the last sample loses its last 256 pixels
        ex = excess("grid_stride", (rot, pad, ac), (None, None, dropped), ("dpose",))
        _report(6, "d pose without the last 256-pixel block (%s, %s, align %d)" % (rot, pad, ac), ex)
        assert ex["dpose"] >= REJECT


def _photo_variant(name, rot, pad, ac, with_mask, oob_mask=True, shift=0):
    """oracle.losses.photometric_reconstruction_loss in fp64 with two switches: (loss, dpose)"""
    i = GA.photo_inputs(name)
    pose = GA._leaf(i["pose"], F64)
    masks = [m.double() for m in GA.photo_masks(name, rot, ac)] if with_mask else [None] * len(i["depth"])
    refs = [torch.roll(r.double(), shift, dims=3) for r in i["refs"]]
    tgt, K, Kinv = i["tgt"].double(), i["K"].double(), i["Kinv"].double()
    if oob_mask:
        v = OL.photometric_reconstruction_loss(tgt, refs, K, Kinv, [d.double() for d in i["depth"]], masks, pose, rot, pad, ac)
    else:
        v = 0
        for d, m in zip(i["depth"], masks):
            h, w = d.shape[2:]
            ks, kinvs = GA._scaled_intrinsics(K, Kinv, tgt.shape[2] / h)
            tgt_s = F.interpolate(tgt, (h, w), mode="area")
            for r, ref in enumerate(refs):
                diff = tgt_s - OG.inverse_warp(F.interpolate(ref, (h, w), mode="area"), d[:, 0].double(), pose[:, r], ks, kinvs, rot, pad, ac)
                v = v + (diff if m is None else diff * m[:, r:r + 1]).abs().mean()
    v.backward()
    return v.detach(), pose.grad


def _photo_excess(mode, got_loss, got_dpose):
    rot, pad, ac, with_mask = mode
    r64, r32 = GA.photo_reference("photo_3ref", *mode, F64), GA.photo_reference("photo_3ref", *mode, F32)
    la, pa = (0.0, 0.0) if with_mask else GA.photo_allowance("photo_3ref", rot, pad, ac)[:2]
    ex = {"loss": GA.compare("loss", got_loss, r64[0], r32[0], extra=la).excess}
    if with_mask:
        ex["dpose"] = GA.compare("dpose", got_dpose, r64[2], r32[2]).excess
    return ex


def test_photo_variant_passes():
    for mode in GA.PHOTO_MODES:
        ex = _photo_excess(mode, *_photo_variant("photo_3ref", *mode))
        assert max(ex.values()) <= 1.0, (mode, ex)


def test_mutant_07_photometric_without_the_out_of_bounds_mask():
    for mode in GA.PHOTO_MODES:
        if mode[1] != "zeros":
            continue                                              # border padding never produces an all-zero pixel
        ex = _photo_excess(mode, *_photo_variant("photo_3ref", *mode, oob_mask=False))
        _report(7, "photometric term without the warped == 0 mask %s" % (mode,), ex)
        assert ex["loss"] >= REJECT


def test_mutant_08_source_shifted_by_one_pixel():
    for rot, pad, ac in GA.WARP_MODES:
        got = run_warp("oob_ragged", rot, ac, lambda img, *a: OG.inverse_warp(torch.roll(img, 1, dims=3), *a, rot, pad, ac))
        ex = excess("oob_ragged", (rot, pad, ac), got)
        _report(8, "source image shifted by one pixel in x (%s, %s, align %d)" % (rot, pad, ac), ex)
        assert min(ex.values()) >= REJECT
    for mode in GA.PHOTO_MODES:                                   # (without a mask the loss of random images barely moves: not asserted)
        ex = _photo_excess(mode, *_photo_variant("photo_3ref", *mode, shift=1))
        _report(8, "reference images shifted by one pixel in x %s" % (mode,), ex)
        assert min(ex.values()) >= REJECT or not mode[3]


def _ssim_replicate(x, y):
    pad = lambda t: F.pad(t, (1, 1, 1, 1), mode="replicate")
    x, y = pad(x), pad(y)
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sig_x, sig_y, sig_xy = F.avg_pool2d(x * x, 3, 1) - mu_x ** 2, F.avg_pool2d(y * y, 3, 1) - mu_y ** 2, F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + OI.SSIM_C1) * (2 * sig_xy + OI.SSIM_C2)
    d = (mu_x ** 2 + mu_y ** 2 + OI.SSIM_C1) * (sig_x + sig_y + OI.SSIM_C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def test_mutant_09_ssim_reflection_replaced_by_replication():
    c = GA.CASES["ssim_min"]
    for planes in c["planes"]:
        for size in c["sizes"]:
            x, y, g = GA.ssim_inputs(planes, size)
            r64, r32 = GA.ssim_reference(planes, size, F64), GA.ssim_reference(planes, size, F32)
            for k, q in enumerate(("ssim", "dx", "dy")):          # the oracle in fp32 passes
                assert GA.compare(q, r32[k], r64[k], r32[k]).excess <= 1.0
            xl, yl = GA._leaf(x, F64), GA._leaf(y, F64)
            s = _ssim_replicate(xl, yl)
            (s * g.double()).sum().backward()
            ex = {q: GA.compare(q, t, r64[k], r32[k]).excess for k, (q, t) in enumerate((("ssim", s), ("dx", xl.grad), ("dy", yl.grad)))}
            _report(9, "SSIM border replicated, planes %s size %s" % (planes, size), ex)
            assert min(ex.values()) >= REJECT


class _AbsSign1(torch.autograd.Function):
    """|v| with sgn(0) := 1 in the backward"""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return v.abs()

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return g * torch.where(v >= 0, torch.ones_like(v), -torch.ones_like(v))


def _smooth2_sign1(m):
    dy = m[:, :, 1:] - m[:, :, :-1]
    dx = m[:, :, :, 1:] - m[:, :, :, :-1]
    terms = (dx[:, :, :, 1:] - dx[:, :, :, :-1], dx[:, :, 1:] - dx[:, :, :-1], dy[:, :, :, 1:] - dy[:, :, :, :-1], dy[:, :, 1:] - dy[:, :, :-1])
    return sum(_AbsSign1.apply(t).mean() for t in terms)


def test_mutant_10_smooth2_sign_of_zero():
    for shape in GA.CASES["smooth_min"]["shapes"]:
        m0 = GA.smooth_inputs(shape, True)
        _, g64 = GA.smooth_reference(shape, True, F64)
        _, g32 = GA.smooth_reference(shape, True, F32)
        tol = GA.sign_exact_tol(shape)
        assert float((g32.double() - g64).abs().max()) <= tol      # an honest fp32 gradient is 'exact' in the stated sense
        m = GA._leaf(m0, F64)
        _smooth2_sign1(m).backward()
        ex = float((m.grad - g64).abs().max()) / tol
        dy, dx = m0[:, :, 1:] - m0[:, :, :-1], m0[:, :, :, 1:] - m0[:, :, :, :-1]
        ties = sum(int((t == 0).sum()) for t in (dx[:, :, :, 1:] - dx[:, :, :, :-1], dx[:, :, 1:] - dx[:, :, :-1], dy[:, :, 1:] - dy[:, :, :-1]))
        _report(10, "smooth2 gradient with sgn(0) := 1, map %s (%d exact ties)" % (shape, ties), {"grad": ex})
        assert ties > 0 and ex >= REJECT
        # the same on the edge-aware smoothness: a plateau disparity, measured tolerance
    for planes in GA.CASES["edge_min"]["planes"]:
        for size in GA.CASES["edge_min"]["sizes"]:
            disp, img = GA.edge_inputs(planes, size, True)
            r64, r32 = GA.edge_reference(planes, size, True, F64), GA.edge_reference(planes, size, True, F32)
            assert GA.compare("edge", r32[1], r64[1], r32[1]).excess <= 1.0
            d = GA._leaf(disp, F64)
            gdx, gdy = _AbsSign1.apply(d[:, :, :, :-1] - d[:, :, :, 1:]), _AbsSign1.apply(d[:, :, :-1] - d[:, :, 1:])
            i64 = img.double()
            gix = (i64[:, :, :, :-1] - i64[:, :, :, 1:]).abs().mean(1, keepdim=True)
            giy = (i64[:, :, :-1] - i64[:, :, 1:]).abs().mean(1, keepdim=True)
            ((gdx * torch.exp(-gix)).mean() + (gdy * torch.exp(-giy)).mean()).backward()
            ex = GA.compare("edge", d.grad, r64[1], r32[1]).excess
            ties = int((disp[:, :, :, :-1] == disp[:, :, :, 1:]).sum() + (disp[:, :, :-1] == disp[:, :, 1:]).sum())
            _report(10, "edge smoothness with sgn(0) := 1, planes %s size %s (%d ties)" % (planes, size, ties), {"grad": ex})
            assert ex >= REJECT or ties == 0
