"""numpy restatement of the random scale-and-crop contract (include/dispnet_hip.h above dn_scale_crop_minmax), built
on tests/pil_resize.py and written from the algorithm, independent of supervised_dispnet_amd/data.py and shards.py: the FULL scaled image
is computed, then cropped.  tests/test_scale_crop_host.py holds it to Pillow itself; the GPU tests hold the kernels to it."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from pil_resize import bytescale, resample_axis  # noqa: E402


def draws(rng, H, W):
    """The four numpy calls of the reference's RandomScaleCrop, in its order -> (sx, sy, sh, sw, oy, ox)."""
    sx, sy = rng.uniform(1, 1.15, 2)
    sh, sw = int(H * sy), int(W * sx)
    oy = rng.randint(sh - H + 1)
    ox = rng.randint(sw - W + 1)
    return sx, sy, sh, sw, oy, ox


def scaled_u8(a, sh, sw):
    """Byte-scale (always), then Pillow's two passes, each skipped for an axis that keeps its size.  a: [H, W, 3] or [H, W], any values."""
    u8 = bytescale(a)
    if sw != u8.shape[1]:
        u8 = resample_axis(u8, sw, 1)
    if sh != u8.shape[0]:
        u8 = resample_axis(u8, sh, 0)
    return u8


def image(frame_u8, flip, sh, sw, oy, ox, mean, std):
    """uint8 [H, W, 3] -> (uint8 crop [H, W, 3], normalised fp32 [3, H, W])."""
    H, W = frame_u8.shape[:2]
    f = frame_u8[:, ::-1] if flip else frame_u8
    u8 = scaled_u8(f.astype(np.float32), sh, sw)[oy:oy + H, ox:ox + W]
    x = np.transpose(u8, (2, 0, 1)).astype(np.float32) / np.float32(255)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    return u8, ((x - m) / s).astype(np.float32)


def depth(d, flip, sh, sw, oy, ox):
    """fp32 [H, W] -> fp32 [H, W]: byte-scale over the map's own min / max, the two passes, fp32(fp64(u8) / 255.0 * fp64(max))."""
    d = np.asarray(d, dtype=np.float32)
    H, W = d.shape
    f = d[:, ::-1] if flip else d
    gmax = np.float64(np.float32(f.max()))
    u8 = scaled_u8(f, sh, sw)[oy:oy + H, ox:ox + W]
    return (u8.astype(np.float64) / 255.0 * gmax).astype(np.float32)


def intrinsics(k, W, flip, sx, sy, oy, ox):
    """fp32 [3, 3] -> fp32 [3, 3]: the flip rule, then every product and difference in fp64, rounded to fp32 once each."""
    k = np.array(k, dtype=np.float32)
    if flip:
        k[0, 2] = np.float32(W) - k[0, 2]
    for j in range(3):
        k[0, j] = np.float32(np.float64(k[0, j]) * np.float64(sx))
        k[1, j] = np.float32(np.float64(k[1, j]) * np.float64(sy))
    k[0, 2] = np.float32(np.float64(k[0, 2]) - np.float64(ox))
    k[1, 2] = np.float32(np.float64(k[1, 2]) - np.float64(oy))
    return k
