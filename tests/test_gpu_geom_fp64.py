"""The warp / photometric / smoothness kernels (csrc/dn_warp.hip, smooth2 of csrc/dn_loss.hip) against the fp64 oracle, on the cases of
tests/geom_audit.py: inputs that drive the zeros substitution, the border clip, the Z clamp gate, the grid-stride loop, three
reference images over four scales, and the minimum sizes of SSIM and the smoothness terms.  pytest -m gpu.

Every tolerance is geom_audit.check(): MARGIN x the fp32 CPU oracle's own error against fp64 on the same inputs, fragile pixels
removed beforehand (tests/test_geom_audit_host.py shows what that rejects).  Each comparison prints its figures; the worst per
quantity are recorded in geom_audit's docstring.
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

import geom_audit as GA  # noqa: E402
import supervised_dispnet_amd.inverse_warp as IW  # noqa: E402
import supervised_dispnet_amd.layers as L  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
from supervised_dispnet_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
DN_ERR_BAD_ARG = -1


def dev(t):
    return t.to(DEV)


def _gpu_warp(name, rot, pad, ac):
    i = GA.warp_inputs(name)
    keep = ~GA.fragile(name, rot, ac)[:, None]
    d, p = dev(i["depth"]).requires_grad_(), dev(i["pose"]).requires_grad_()
    out = IW.inverse_warp(dev(i["img"]), d, p, dev(i["K"]), dev(i["Kinv"]), rot, pad, align_corners=ac)
    (out * dev(i["gw"] * keep)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), d.grad, p.grad


@pytest.mark.parametrize("name", GA.WARP_CASES)
def test_inverse_warp_vs_fp64(name):
    for mode in GA.WARP_MODES:
        r64, r32 = GA.warp_reference(name, *mode, F64), GA.warp_reference(name, *mode, F32)
        got = _gpu_warp(name, *mode)
        tag = "%s:%s:%s:ac%d" % ((name,) + (mode[0], mode[1], int(mode[2])))
        GA.check(tag + ":warped", got[0], r64[0], r32[0], keep=r64[3])
        GA.check(tag + ":ddepth", got[1], r64[1], r32[1])
        GA.check(tag + ":dpose", got[2], r64[2], r32[2])


def _gpu_photo(rot, pad, ac, with_mask):
    i = GA.photo_inputs("photo_3ref")
    depth = [dev(d).requires_grad_() for d in i["depth"]]
    pose = dev(i["pose"]).requires_grad_()
    masks = [dev(m).requires_grad_() for m in GA.photo_masks("photo_3ref", rot, ac)] if with_mask else [None] * len(depth)
    v = LF.photometric_reconstruction_loss(dev(i["tgt"]), [dev(r) for r in i["refs"]], dev(i["K"]), dev(i["Kinv"]), depth, masks, pose,
                                           rot, pad, align_corners=ac)
    v.backward()
    torch.cuda.synchronize()
    return v.detach(), [d.grad for d in depth], pose.grad, [m.grad for m in masks] if with_mask else None


@pytest.mark.parametrize("mode", GA.PHOTO_MODES, ids=lambda m: "%s-%s-ac%d-mask%d" % (m[0], m[1], m[2], m[3]))
def test_photometric_3ref_vs_fp64(mode):
    rot, pad, ac, with_mask = mode
    r64, r32 = GA.photo_reference("photo_3ref", *mode, F64), GA.photo_reference("photo_3ref", *mode, F32)
    got = _gpu_photo(*mode)
    tag = "photo_3ref:%s:%s:ac%d:mask%d" % (rot, pad, ac, with_mask)
    if with_mask:                   # the fragile pixels carry a zero mask: nothing to allow for
        loss_allow, pose_allow, keeps = 0.0, None, [None] * len(got[1])
    else:
        loss_allow, pose_allow, keeps = GA.photo_allowance("photo_3ref", rot, pad, ac)
    GA.check(tag + ":loss", got[0], r64[0], r32[0], extra=loss_allow)
    for s in range(len(got[1])):
        GA.check(tag + ":ddepth%d" % s, got[1][s], r64[1][s], r32[1][s], keep=keeps[s])
    if with_mask:                   # the strict pose comparison: all three references, no allowance
        GA.check(tag + ":dpose", got[2], r64[2], r32[2])
    else:                           # per component: the allowance differs by orders of magnitude between translation and rotation
        for r in range(got[2].shape[1]):
            for k in range(6):
                GA.check(tag + ":dpose[ref%d][%d]" % (r, k), got[2][:, r, k], r64[2][:, r, k], r32[2][:, r, k], extra=float(pose_allow[r, k]),
                         verbose=False)
    if with_mask:
        for s in range(len(got[3])):
            GA.check(tag + ":dmask%d" % s, got[3][s], r64[3][s], r32[3][s])


def test_pose_matrices_big_angles_vs_fp64():
    vec, wt = GA.pose_vectors(), GA.pose_weight()
    for rot in GA.ROTS:
        r64, r32 = GA.pose_reference(rot, F64), GA.pose_reference(rot, F32)
        v = dev(vec).requires_grad_()
        m = IW.pose_vec2mat(v, rot)
        (m * dev(wt)).sum().backward()
        a = dev(vec[:, 3:]).requires_grad_()
        r = (IW.euler2mat if rot == "euler" else IW.quat2mat)(a)
        (r * dev(wt[:, :, :3])).sum().backward()
        for k, (q, t) in enumerate((("pose_vec2mat", m), ("d pose_vec2mat", v.grad), ("%s2mat" % rot, r), ("d %s2mat" % rot, a.grad))):
            GA.check("big_angles:%s:%s" % (rot, q), t, r64[k], r32[k])


def test_ssim_minimum_sizes_vs_fp64():
    c = GA.CASES["ssim_min"]
    for planes in c["planes"]:
        for size in c["sizes"]:
            x, y, g = GA.ssim_inputs(planes, size)
            r64, r32 = GA.ssim_reference(planes, size, F64), GA.ssim_reference(planes, size, F32)
            xd, yd = dev(x).requires_grad_(), dev(y).requires_grad_()
            s = L.SSIM()(xd, yd)
            (s * dev(g)).sum().backward()
            tag = "ssim_min:%dx%d:%dx%d" % (planes + size)
            GA.check(tag + ":ssim", s, r64[0], r32[0])
            GA.check(tag + ":dx", xd.grad, r64[1], r32[1])
            GA.check(tag + ":dy", yd.grad, r64[2], r32[2])


def test_ssim_of_identical_images_is_exactly_zero():
    c = GA.CASES["ssim_min"]
    for planes in c["planes"]:
        for size in c["sizes"] + ((20, 28),):
            x, y, _ = GA.ssim_inputs(planes, size, same=True)
            s = L.SSIM()(dev(x), dev(y))
            print("geom_audit ssim(x, x) %s %s: max %.3e, %d of %d non-zero" % (planes, size, float(s.max()), int((s != 0).sum()), s.numel()))
            assert float(s.abs().max()) == 0.0, (planes, size, float(s.abs().max()))


def test_edge_smoothness_minimum_sizes_vs_fp64():
    c = GA.CASES["edge_min"]
    for planes in c["planes"]:
        for size in c["sizes"]:
            for flat in (False, True):
                disp, img = GA.edge_inputs(planes, size, flat)
                r64, r32 = GA.edge_reference(planes, size, flat, F64), GA.edge_reference(planes, size, flat, F32)
                d = dev(disp).requires_grad_()
                v = L.get_smooth_loss(d, dev(img))
                v.backward()
                tag = "edge_min:%dx%d:%dx%d:%s" % (planes + size + ("plateau" if flat else "uniform",))
                GA.check(tag + ":loss", v, r64[0], r32[0])
                GA.check(tag + ":ddisp", d.grad, r64[1], r32[1])


@pytest.mark.parametrize("fn", ("smooth_loss", "smooth_DORN_loss"))
def test_second_order_smoothness_minimum_sizes_vs_fp64(fn):
    for shape in GA.CASES["smooth_min"]["shapes"]:
        for flat in (False, True):
            r64, r32 = GA.smooth_reference(shape, flat, F64), GA.smooth_reference(shape, flat, F32)
            m = dev(GA.smooth_inputs(shape, flat)).requires_grad_()
            v = getattr(LF, fn)(m)
            v.backward()
            tag = "smooth_min:%s:%dx%dx%dx%d:%s" % ((fn,) + tuple(shape) + ("plateau" if flat else "uniform",))
            GA.check(tag + ":loss", v, r64[0], r32[0])
            if flat:                # exact second differences: every sign, sgn(0) = 0 included, must be the fp64 one
                err, tol = float((m.grad.double().cpu() - r64[1]).abs().max()), GA.sign_exact_tol(shape)
                print("geom_audit %-44s err %.3e rounding allowance %.3e (one sign: %.3e)" % (
                    tag + ":dmap", err, tol, 1.0 / (shape[0] * shape[1] * shape[2] * shape[3])))
                assert err <= tol, (tag, err, tol)
            else:
                GA.check(tag + ":dmap", m.grad, r64[1], r32[1])


def test_smooth_loss_scale_weights_vs_fp64():
    """a list of maps: the per-scale weights 1, 1 / 2.3, 1 / 2.3^2 of one autograd node"""
    shapes = GA.CASES["smooth_min"]["shapes"][1:]
    from oracle import losses as OL
    refs = {}
    for dt in (F64, F32):
        ms = [GA._leaf(GA.smooth_inputs(s, False), dt) for s in shapes]
        v = OL.smooth_loss(ms)
        v.backward()
        refs[dt] = (v.detach(), [m.grad for m in ms])
    ms = [dev(GA.smooth_inputs(s, False)).requires_grad_() for s in shapes]
    v = LF.smooth_loss(ms)
    v.backward()
    GA.check("smooth_min:list:loss", v, refs[F64][0], refs[F32][0])
    for k, m in enumerate(ms):
        GA.check("smooth_min:list:dmap%d" % k, m.grad, refs[F64][1][k], refs[F32][1][k])


def test_warp_and_photometric_are_deterministic():
    """'No atomics (deterministic)': forward and backward twice, every output bit for bit"""
    for mode in GA.WARP_MODES:
        a, b = _gpu_warp("grid_stride", *mode), _gpu_warp("grid_stride", *mode)
        for u, v in zip(a, b):
            assert torch.equal(u, v), ("grid_stride", mode)
    for mode in GA.PHOTO_MODES:
        a, b = _gpu_photo(*mode), _gpu_photo(*mode)
        flat = lambda r: [r[0]] + list(r[1]) + [r[2]] + list(r[3] or [])
        for u, v in zip(flat(a), flat(b)):
            assert torch.equal(u, v), ("photo_3ref", mode)


def test_abi_argument_checks():
    """argument checks of the C ABI that run no kernel: a 1-row warp or SSIM, an area factor that does not divide the size"""
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = t.data_ptr()
    assert lib.dn_inverse_warp_fwd(p, p, p, p, 1, 1, 4, 0, 0, p, None) == DN_ERR_BAD_ARG
    assert lib.dn_inverse_warp_fwd(p, p, p, p, 1, 4, 1, 0, 0, p, None) == DN_ERR_BAD_ARG
    assert lib.dn_inverse_warp_fwd(p, p, p, p, 1, 2, 2, 2, 0, p, None) == DN_ERR_BAD_ARG         # padding mode 2
    assert lib.dn_ssim_fwd(p, p, 1, 1, 4, p, None) == DN_ERR_BAD_ARG
    assert lib.dn_ssim_fwd(p, p, 1, 4, 1, p, None) == DN_ERR_BAD_ARG
    assert lib.dn_area_down(p, 1, 6, 8, 4, p, None) == DN_ERR_BAD_ARG
    assert lib.dn_area_down(p, 1, 8, 6, 4, p, None) == DN_ERR_BAD_ARG
    assert lib.dn_smooth2_fwd(p, 1, 2, 3, 1.0, p, p, None) == DN_ERR_BAD_ARG
    assert "dn_smooth2_fwd" in _lib.last_error()
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0                               # nothing was launched on the buffer
