"""Mirror of the hot-path pieces of the reference's layers.py on HIP kernels: SSIM, get_smooth_loss, disp_to_depth, the pose / geometry
layers of the self-supervised loss (transformation_from_parameters, BackprojectDepth, Project3D) and the monodepth2 building blocks
(ConvBlock / Conv3x3 / upsample) used by networks.DepthDecoder.
"""
import torch
import torch.nn as nn

from . import _lib
from .engine import _ptr, _stream, require_cuda


def disp_to_depth(disp, min_depth, max_depth):
    """reference layers.py:14-24 (host-side scalar arithmetic on the network output; not a kernel in the reference either)."""
    min_disp = 1 / max_depth
    max_disp = 1 / min_depth
    scaled_disp = min_disp + (max_disp - min_disp) * disp
    depth = 1 / scaled_disp
    return scaled_disp, depth


def _vec3(t, what):
    """(tensor, batch stride, element stride) of a [B, ..., 3] vector batch read in place through its strides (normally a view of the
    pose network's [B, F, 1, 6] output: no contiguous copy)."""
    require_cuda(t, what)
    if t.dtype != torch.float32 or t.shape[-1] != 3 or t.numel() != 3 * t.shape[0]:
        raise ValueError("%s: expected a float32 [B, 1, 3] tensor, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t, t.stride(0), t.stride(-1)


class _PoseMatrix(torch.autograd.Function):
    """mode 0: rot_from_axisangle, 1: get_translation_matrix, 2: transformation_from_parameters (dn_pose_matrix_fwd / _bwd: one thread
    per batch element)."""

    @staticmethod
    def forward(ctx, mode, invert, axisangle, translation):
        ref = axisangle if axisangle is not None else translation
        b = ref.shape[0]
        aa = _vec3(axisangle, "axisangle") if axisangle is not None else (None, 0, 0)
        tr = _vec3(translation, "translation") if translation is not None else (None, 0, 0)
        m = torch.empty((b, 4, 4), dtype=torch.float32, device=ref.device)
        args = (_ptr(aa[0]), aa[1], 0, aa[2], _ptr(tr[0]), tr[1], 0, tr[2], b, 1, mode, 1 if invert else 0)
        _lib.call("dn_pose_matrix_fwd", *args, m.data_ptr(), _stream())
        ctx.args, ctx.keep = args, (axisangle, translation)
        return m

    @staticmethod
    def backward(ctx, dm):
        axisangle, translation = ctx.keep
        g = dm.contiguous().float()
        daa = torch.empty(axisangle.shape, dtype=torch.float32, device=g.device) if axisangle is not None and ctx.needs_input_grad[2] else None
        dtr = torch.empty(translation.shape, dtype=torch.float32, device=g.device) if translation is not None and ctx.needs_input_grad[3] else None
        _lib.call("dn_pose_matrix_bwd", *ctx.args, g.data_ptr(), _ptr(daa), _ptr(dtr), _stream())
        return None, None, daa, dtr


def rot_from_axisangle(vec):
    """reference layers.py:64-103: `vec` [B,1,3] -> [B,4,4]; angle = |v|, axis = v / (angle + 1e-7), Rodrigues."""
    return _PoseMatrix.apply(0, False, vec, None)


def get_translation_matrix(translation_vector):
    """reference layers.py:48-61: [B,1,3] (any shape holding 3 values per batch element) -> [B,4,4]."""
    return _PoseMatrix.apply(1, False, None, translation_vector)


def transformation_from_parameters(axisangle, translation, invert=False):
    """reference layers.py:28-45: M = T R, or R^T T(-t) with `invert`."""
    return _PoseMatrix.apply(2, bool(invert), axisangle, translation)


class _Backproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, inv_K, b, h, w):
        require_cuda(depth, "depth")
        require_cuda(inv_K, "inv_K")
        dc, kc = depth.contiguous().float(), inv_K.contiguous().float()
        if dc.numel() != b * h * w or tuple(kc.shape) != (b, 4, 4):
            raise ValueError("BackprojectDepth(%d, %d, %d): got depth %s, inv_K %s" % (b, h, w, tuple(depth.shape), tuple(inv_K.shape)))
        out = torch.empty((b, 4, h * w), dtype=torch.float32, device=dc.device)
        _lib.call("dn_backproject_fwd", dc.data_ptr(), kc.data_ptr(), b, h, w, out.data_ptr(), _stream())
        ctx.save_for_backward(kc)
        ctx.cfg = (b, h, w, depth.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        (kc,) = ctx.saved_tensors
        b, h, w, shape = ctx.cfg
        g = dout.contiguous().float()
        dd = torch.empty(shape, dtype=torch.float32, device=g.device)
        _lib.call("dn_backproject_bwd", g.data_ptr(), kc.data_ptr(), b, h, w, dd.data_ptr(), _stream())
        return dd, None, None, None, None


class BackprojectDepth(nn.Module):
    """reference layers.py:139-165: depth [B,1,H,W] -> point cloud [B,4,H*W]; the gradient flows to the depth.  The pixel grid is
    computed in the kernel and the module holds no parameters (the reference registers its constant grids as trainable
    nn.Parameters, and its forward stops in an unimported pdb: neither is reproduced)."""

    def __init__(self, batch_size, height, width):
        super(BackprojectDepth, self).__init__()
        self.batch_size, self.height, self.width = batch_size, height, width

    def forward(self, depth, inv_K):
        return _Backproject.apply(depth, inv_K, self.batch_size, self.height, self.width)


class _Project3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, K, T, b, h, w, eps):
        for t, what in ((points, "points"), (K, "K"), (T, "T")):
            require_cuda(t, what)
        pc, kc, tc = points.contiguous().float(), K.contiguous().float(), T.contiguous().float()
        if tuple(pc.shape) != (b, 4, h * w) or tuple(kc.shape) != (b, 4, 4) or tuple(tc.shape) != (b, 4, 4):
            raise ValueError("Project3D(%d, %d, %d): got points %s, K %s, T %s" % (b, h, w, tuple(points.shape), tuple(K.shape), tuple(T.shape)))
        grid = torch.empty((b, h, w, 2), dtype=torch.float32, device=pc.device)
        _lib.call("dn_project3d_fwd", pc.data_ptr(), kc.data_ptr(), tc.data_ptr(), b, h, w, eps, grid.data_ptr(), _stream())
        ctx.save_for_backward(pc, kc, tc)
        ctx.cfg = (b, h, w, eps)
        return grid

    @staticmethod
    def backward(ctx, dgrid):
        pc, kc, tc = ctx.saved_tensors
        b, h, w, eps = ctx.cfg
        g = dgrid.contiguous().float()
        dp = torch.empty_like(pc)
        dt = torch.empty_like(tc)
        partial = torch.empty(b * _lib.load().dn_reproj_blocks(h, w) * 12, dtype=torch.float32, device=g.device)
        _lib.call("dn_project3d_bwd", pc.data_ptr(), kc.data_ptr(), tc.data_ptr(), g.data_ptr(), b, h, w, eps, dp.data_ptr(), partial.data_ptr(),
                  dt.data_ptr(), _stream())
        return dp, None, dt, None, None, None, None


class Project3D(nn.Module):
    """reference layers.py:168-190: points [B,4,H*W] -> sampling grid [B,H,W,2] in [-1, 1]; no clamp on the projected depth (this is
    where it differs from inverse_warp).  Gradients flow to the points and to T."""

    def __init__(self, batch_size, height, width, eps=1e-7):
        super(Project3D, self).__init__()
        self.batch_size, self.height, self.width, self.eps = batch_size, height, width, eps

    def forward(self, points, K, T):
        return _Project3D.apply(points, K, T, self.batch_size, self.height, self.width, self.eps)


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        require_cuda(x, "SSIM input x")
        require_cuda(y, "SSIM input y")
        xc, yc = x.contiguous().float(), y.contiguous().float()
        if xc.shape != yc.shape or xc.dim() != 4:
            raise ValueError("SSIM expects two [B,C,H,W] tensors of the same shape")
        b, c, h, w = xc.shape
        out = torch.empty_like(xc)
        _lib.call("dn_ssim_fwd", xc.data_ptr(), yc.data_ptr(), b * c, h, w, out.data_ptr(), _stream())
        ctx.save_for_backward(xc, yc)
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, yc = ctx.saved_tensors
        b, c, h, w = xc.shape
        g = dout.contiguous().float()
        ws = torch.empty(5 * xc.numel(), dtype=torch.float32, device=xc.device)
        dx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(yc) if ctx.needs_input_grad[1] else None
        _lib.call("dn_ssim_bwd", xc.data_ptr(), yc.data_ptr(), g.data_ptr(), b * c, h, w, ws.data_ptr(),
                  dx.data_ptr() if dx is not None else None, dy.data_ptr() if dy is not None else None, _stream())
        return dx, dy


class SSIM(nn.Module):
    """reference layers.py:215-245: ReflectionPad2d(1) + 3x3 means, C1 = 0.01^2, C2 = 0.03^2, clamp((1 - SSIM)/2, 0, 1)."""

    def __init__(self):
        super(SSIM, self).__init__()
        self.C1 = 0.01 ** 2
        self.C2 = 0.03 ** 2

    def forward(self, x, y):
        return _SSIM.apply(x, y)


class _EdgeSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img):
        require_cuda(disp, "disparity")
        require_cuda(img, "image")
        dc, ic = disp.contiguous().float(), img.contiguous().float()
        b, c1, h, w = dc.shape
        if c1 != 1:
            raise ValueError("get_smooth_loss expects a 1-channel disparity, got %d channels" % c1)
        c = ic.shape[1]
        nb = _lib.load().dn_edge_smooth_blocks(b, h, w)
        partial = torch.empty((nb, 2), dtype=torch.float32, device=dc.device)
        loss = torch.empty((), dtype=torch.float32, device=dc.device)
        _lib.call("dn_edge_smooth_fwd", dc.data_ptr(), ic.data_ptr(), b, c, h, w, partial.data_ptr(), loss.data_ptr(), _stream())
        ctx.save_for_backward(dc, ic)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dc, ic = ctx.saved_tensors
        b, _, h, w = dc.shape
        dl = dloss.contiguous().float()
        g = torch.empty_like(dc)
        _lib.call("dn_edge_smooth_bwd", dc.data_ptr(), ic.data_ptr(), dl.data_ptr(), b, ic.shape[1], h, w, g.data_ptr(), _stream())
        return g, None


def get_smooth_loss(disp, img):
    """reference layers.py:199-212: edge-aware first-order smoothness (gradient w.r.t. the disparity)."""
    return _EdgeSmooth.apply(disp, img)


def upsample(x):
    """reference layers.py:193-196 (nearest x2).  Inside networks.DepthDecoder the upsample is virtual (the consumer conv's
    loader reads index >> 1); this standalone form is kept for API completeness and is not on the hot path."""
    raise NotImplementedError("layers.upsample is fused into the consumer convolution on the HIP path (networks.DepthDecoder)")


class Conv3x3(nn.Module):
    """reference layers.py:124-136: ReflectionPad2d(1) (or ZeroPad2d) + Conv2d(3x3).  Parameter container: executed by
    networks.DepthDecoder through the engine (reflection is a loader index map, not a padded copy)."""

    def __init__(self, in_channels, out_channels, use_refl=True):
        super(Conv3x3, self).__init__()
        self.pad = nn.ReflectionPad2d(1) if use_refl else nn.ZeroPad2d(1)
        self.conv = nn.Conv2d(int(in_channels), int(out_channels), 3)


class ConvBlock(nn.Module):
    """reference layers.py:106-121: Conv3x3 + ELU (parameter container, see Conv3x3)."""

    def __init__(self, in_channels, out_channels):
        super(ConvBlock, self).__init__()
        self.conv = Conv3x3(in_channels, out_channels)
        self.nonlin = nn.ELU(inplace=True)
