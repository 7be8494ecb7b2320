"""numpy restatements of the host image arithmetic that csrc/dn_image.hip reproduces, written from the
algorithms and independent of supervised_dispnet_amd/inference.py: scipy.misc.imresize = byte-scale + Pillow's 8-bit bilinear resize,
PIL.ImageEnhance.Contrast, and the colouring of utils.tensor2array.  tests/test_image_host.py holds them to Pillow itself; the GPU
tests then hold the kernels to the host libraries."""
import numpy as np

PRECISION_BITS = 22


def bytescale(a):
    """float32 frame -> uint8 by its own min / max over all channels (numpy float32 arithmetic with Python scalars)."""
    a = np.asarray(a, dtype=np.float32)
    cmin, cmax = float(a.min()), float(a.max())
    scale = 255.0 / (cmax - cmin) if cmax > cmin else 1.0
    t = np.float32(np.float32(a - np.float32(cmin)) * np.float32(scale)) + np.float32(0.5)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def coefficients(n, O):
    """[(first input index, int64 coefficients)] per output index of one axis."""
    scale = n / O
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    rows = []
    for o in range(O):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        last = min(int(center + support + 0.5), n)
        wgt = [max(0.0, 1.0 - abs((x + first - center + 0.5) * ss)) for x in range(last - first)]
        total = 0.0
        for v in wgt:
            total += v
        rows.append((first, np.array([int(v / total * (1 << PRECISION_BITS) + 0.5) for v in wgt], dtype=np.int64)))
    return rows


def resample_axis(a, O, axis):
    a = np.moveaxis(a, axis, 0)
    out = np.empty((O,) + a.shape[1:], np.uint8)
    for o, (first, k) in enumerate(coefficients(a.shape[0], O)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, a[first:first + len(k)].astype(np.int64), 1)
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8(a, h, w):
    """Pillow's Image.resize((w, h), BILINEAR) of a uint8 [H, W, 3] array: horizontal pass into uint8, then the vertical pass."""
    if a.shape[1] != w:
        a = resample_axis(a, w, 1)
    if a.shape[0] != h:
        a = resample_axis(a, h, 0)
    return a


def imresize(frame, h, w):
    """scipy.misc.imresize(frame, (h, w)) as the reference calls it: a frame that already has the size is not touched."""
    frame = np.asarray(frame)
    if frame.shape[:2] == (h, w):
        return frame.astype(np.uint8)
    return resize_u8(bytescale(frame), h, w)


def contrast(im, factor):
    """PIL.ImageEnhance.Contrast(im).enhance(factor) of a uint8 [h, w, 3] array."""
    i = im.astype(np.int64)
    luma = (i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16
    m = np.float32(int(int(luma.sum()) / luma.size + 0.5))
    t = m + np.float32(factor) * (im.astype(np.float32) - m)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def colorize(x, max_value=None, table=None):
    """(255 * tensor2array(x, max_value, channel_first=False)).astype(uint8) of a float32 [h, w] map; table: uint8 [256, 3] or None (grey).
    A NaN (inf / inf) gives index / grey 0, which is what dn_colorize_u8 defines (numpy's cast of a NaN is left to the platform)."""
    x = np.asarray(x, dtype=np.float32)
    mx = np.float32(x.max() if max_value is None else max_value)
    with np.errstate(invalid="ignore", divide="ignore"):
        if table is not None:
            t = np.float32(np.float32(255) * x) / mx
            index = np.where(np.isnan(t), 0, np.clip(t, 0, 255)).astype(np.uint8)
            return np.asarray(table, dtype=np.uint8)[index]
        g = x / mx
        grey = (np.float32(255) * np.where(np.isnan(g), 0, np.clip(g, 0, 1)).astype(np.float32)).astype(np.uint8)
    return np.repeat(grey[:, :, None], 3, axis=2)
