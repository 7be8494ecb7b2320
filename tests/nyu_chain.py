"""CPU restatement of the NYU Depth v2 transform chain (test infrastructure, fp64 where the reference is fp64).

The reference (datasets/nyu_depth_v2.py:76-110, datasets/image_utils.py) runs, per training sample, on the HWC merge of the
stored (5, H0, W0) float32 array: flip -> scipy.ndimage.rotate(order=3, mode='constant') clipped to the sample's min / max ->
random crop -> skimage warp (bilinear zoom toward the top-left corner, depth / s) -> colour gain on RGB -> ToTensor (no /255) ->
float32 -> Normalize(ImageNet mean / std).  Validation images go through scipy.ndimage.zoom(order=1) to 320x448 and the same
Normalize.  This module restates that chain with scipy.ndimage for rotate and zoom, and `warp_zoom` for skimage's warp (skimage is
not a dependency); `spline_prefilter`, `rotate_restated` and `zoom_restated` spell out what the HIP kernels compute, pinned against
scipy by tests/test_nyu_host.py.

`raw_sample` / `raw_test_images` / `raw_test_depths` generate inputs by formula (oracle.detgen hashes), so the golden file
tests/golden/nyu_transform.npz stores only outputs and draws.
"""
import numpy as np
import scipy.ndimage as ndi

from oracle import detgen

NYUD_MEAN = (0.485, 0.456, 0.406)
NYUD_STD = (0.229, 0.224, 0.225)
POLE = np.sqrt(3.0) - 2.0          # cubic B-spline prefilter pole


# ----------------------------------------------------------------------------- inputs by formula
def _u(shape, tag):
    n = int(np.prod(shape))
    return (detgen._hash_u32(n, detgen.tag_seed(tag)).astype(np.float64) / 4294967296.0).reshape(shape)


def raw_sample(H0, W0, tag):
    """(5, H0, W0) float32 like nyud_raw_train_to_npy.py writes: RGB integers in 0..255, depth in metres, 0/1 mask (depth 0 where
    the mask is 0)."""
    rgb = np.floor(_u((3, H0, W0), tag + ":rgb") * 256.0)
    mask = (_u((1, H0, W0), tag + ":mask") < 0.9).astype(np.float64)
    depth = (0.5 + 9.5 * _u((1, H0, W0), tag + ":depth")) * mask
    return np.concatenate([rgb, depth, mask]).astype(np.float32)


def raw_test_images(n, tag, H=480, W=640):
    return np.floor(_u((n, 3, H, W), tag + ":img") * 256.0).astype(np.float32)


def raw_test_depths(n, tag, H=480, W=640):
    return (0.5 + 9.5 * _u((n, 1, H, W), tag + ":depth")).astype(np.float32)


# ----------------------------------------------------------------------------- restatements of the scipy / skimage steps
def _filter_line(c, z):
    """scipy's order-3 mirror prefilter of one line, in place (gain, causal init + pass, anti-causal init + pass)."""
    n = c.shape[0]
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    z_n_1 = z ** (n - 1)
    c0 = c[0] + z_n_1 * c[n - 1]
    z_i = z
    for i in range(1, n - 1):
        c0 += z_i * (c[i] + z_n_1 * c[n - 1 - i])
        z_i *= z
    c[0] = c0 / (1.0 - z_n_1 * z_n_1)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])


def spline_prefilter(plane):
    """Cubic B-spline coefficients of a 2-D plane with mirror boundaries, fp64, axis 0 then axis 1 (vectorised over the other)."""
    c = np.array(plane, dtype=np.float64)
    for axis in (0, 1):
        v = np.moveaxis(c, axis, 0)          # view: lines along `axis` become v[:, k]
        _filter_line(v, POLE)
    return c


def _mirror(i, n):
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def _cubic_weights(t):
    z = 1.0 - t
    w0 = z * z * z / 6.0
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w3 = 1.0 - w0 - w1 - w2
    return (w0, w1, w2, w3)


def rotation(angle, H, W):
    """scipy.ndimage.rotate's matrix and offset: output (r, c) reads (cs*r + sn*c + off0, -sn*r + cs*c + off1)."""
    a = np.deg2rad(angle)
    cs, sn = np.cos(a), np.sin(a)
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    return cs, sn, cy - (cs * cy + sn * cx), cx - (-sn * cy + cs * cx)


def spline_eval(coef, rr, cc):
    """Order-3 spline value at fp64 source coordinates (arrays): 0 outside [0, H-1] x [0, W-1], mirrored taps at the edges."""
    H, W = coef.shape
    inside = (rr >= 0) & (rr <= H - 1) & (cc >= 0) & (cc <= W - 1)
    rr, cc = np.where(inside, rr, 0.0), np.where(inside, cc, 0.0)
    fr, fc = np.floor(rr), np.floor(cc)
    wy, wx = _cubic_weights(rr - fr), _cubic_weights(cc - fc)
    fr, fc = fr.astype(np.int64), fc.astype(np.int64)
    acc = np.zeros(rr.shape)
    for i in range(4):
        ri = _mirror(fr - 1 + i, H)
        for j in range(4):
            acc = acc + coef[ri, _mirror(fc - 1 + j, W)] * wy[i] * wx[j]
    return np.where(inside, acc, 0.0)


def rotate_restated(plane, angle):
    """scipy.ndimage.rotate(plane, angle, reshape=False, order=3, mode='constant') in fp64 (before the cast to the input dtype)."""
    H, W = plane.shape
    cs, sn, o0, o1 = rotation(angle, H, W)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return spline_eval(spline_prefilter(plane), r * cs + c * sn + o0, r * -sn + c * cs + o1)


def zoom_restated(img, OH, OW):
    """scipy.ndimage.zoom(img, (OH/H, OW/W), order=1) of a 2-D fp32 plane, rounded to fp32: output i reads i*(n_in-1)/(n_out-1)."""
    H, W = img.shape
    zy, zx = (H - 1) / (OH - 1), (W - 1) / (OW - 1)
    y = np.minimum(np.arange(OH) * zy, H - 1)
    x = np.minimum(np.arange(OW) * zx, W - 1)
    y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    wy0, wx0 = 1.0 - (y - y0), 1.0 - (x - x0)
    wy1, wx1 = 1.0 - wy0, 1.0 - wx0
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    a = img.astype(np.float64)
    t = (a[y0][:, x0] * wy0[:, None] * wx0[None, :] + a[y0][:, x1] * wy0[:, None] * wx1[None, :]
         + a[y1][:, x0] * wy1[:, None] * wx0[None, :] + a[y1][:, x1] * wy1[:, None] * wx1[None, :])
    return t.astype(np.float32)


def warp_zoom(image, s):
    """skimage.transform.warp(image, AffineTransform(scale=(s, s)).inverse) restated for an HWC array: output pixel (r, c) reads
    (r * inv, c * inv) with inv = 1/s (the inverse matrix's entry), bilinear (order=1) per channel with skimage's own formula
    ((1-dc)*a + dc*b per row, then (1-dr)*top + dr*bottom; minr = floor, maxr = ceil), cval 0 outside the image, clipped to the input's
    [min, max] (clip=True), float64 output."""
    return warp_scale(image, np.linalg.inv(np.diag([s, s, 1.0]))[0, 0])


def warp_scale(image, inv):
    """warp_zoom with the inverse map's scale entry given: output (r, c) reads (r * inv, c * inv)."""
    a = np.asarray(image, dtype=np.float64)
    H, W = a.shape[:2]
    r, c = np.arange(H) * inv, np.arange(W) * inv
    r0, r1, c0, c1 = np.floor(r), np.ceil(r), np.floor(c), np.ceil(c)
    dr, dc = (r - r0)[:, None, None], (c - c0)[None, :, None]

    def px(ri, ci):
        ri, ci = ri.astype(np.int64), ci.astype(np.int64)
        ok = (ri[:, None] >= 0) & (ri[:, None] < H) & (ci[None, :] >= 0) & (ci[None, :] < W)
        v = a[np.clip(ri, 0, H - 1)][:, np.clip(ci, 0, W - 1)]
        return np.where(ok[:, :, None], v, 0.0)

    top = (1 - dc) * px(r0, c0) + dc * px(r0, c1)
    bottom = (1 - dc) * px(r1, c0) + dc * px(r1, c1)
    return np.clip((1 - dr) * top + dr * bottom, a.min(), a.max())


# ----------------------------------------------------------------------------- the chain
def normalize(rgb_chw_f32):
    """torchvision Normalize on a float32 CHW tensor: (x - mean) / std in fp32."""
    m = np.asarray(NYUD_MEAN, dtype=np.float32)[:, None, None]
    s = np.asarray(NYUD_STD, dtype=np.float32)[:, None, None]
    return ((rgb_chw_f32 - m) / s).astype(np.float32)


def train_chain(raw, p, size=(256, 352)):
    """One training sample: raw (5, H0, W0) float32 and its draws p = (flip, angle, r0, c0, s, mult) ->
    (img (3, th, tw) float32 normalised, depth (th, tw) float32)."""
    flip, angle, r0, c0, s, mult = p
    th, tw = size
    im = np.ascontiguousarray(raw.transpose(1, 2, 0))
    if flip:
        im = im[:, ::-1, :]
    mi, ma = im.min(), im.max()
    im = np.clip(ndi.rotate(im, angle, reshape=False, axes=(0, 1), mode="constant"), mi, ma)
    im = im[int(r0):int(r0) + th, int(c0):int(c0) + tw, :]
    im = warp_zoom(im, s)
    rgb, depth = im[:, :, 0:3], im[:, :, 3] / s
    rgb = np.clip(rgb * mult, 0, 255)
    return normalize(rgb.transpose(2, 0, 1).astype(np.float32)), depth.astype(np.float32)


def val_chain(image, size=(320, 448)):
    """One validation image (3, 480, 640) float32 -> (3, 320, 448) float32 normalised (BilinearResize = ndimage.zoom order 1)."""
    hwc = image.transpose(1, 2, 0)
    z = ndi.zoom(hwc, (size[0] / hwc.shape[0], size[1] / hwc.shape[1], 1), order=1)
    return normalize(np.ascontiguousarray(z.transpose(2, 0, 1)))
