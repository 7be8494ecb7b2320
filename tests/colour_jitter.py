"""monodepth2's colour jitter as arithmetic: a numpy restatement of the four Pillow operations the chain is
made of -- no Pillow in here -- and the builders of the cases tests/test_colour_jitter_host.py and tests/test_gpu_colour_jitter.py share.

  luma        L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16                                   (Pillow's RGB -> L)
  blend       uint8(clip(fp32(a) + fp32(alpha) * (fp32(b) - fp32(a)), 0, 255)), every step rounded to fp32 (no fused multiply-add)
  brightness  blend(0, im, b);  contrast  blend(m, im, c), m = int(sum(L) / N + 0.5);  saturation  blend(L, im, s)
  hue         Pillow's rgb2hsv_row, H = (H + shift) mod 256, Pillow's hsv2rgb -- the round trip is lossy, also for shift 0
A set of parameters is (order, b, c, s, shift) or None (the sample is not jittered), what data.draw_colour_jitter returns.
"""
import itertools

import numpy as np

F32, F64 = np.float32, np.float64


def luma(a):
    a = a.astype(np.uint32)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(a, b, alpha):
    """Image.blend(a, b, alpha) of uint8 arrays (a may be a scalar): numpy rounds the product and the sum to fp32 one by one."""
    a32, b32 = np.asarray(a).astype(F32), np.asarray(b).astype(F32)
    t = a32 + F32(alpha) * (b32 - a32)
    return np.clip(t, 0, 255).astype(np.uint8)


def brightness(im, f):
    return blend(np.uint8(0), im, f)


def contrast_mean(im):
    L = luma(im)
    return int(int(L.astype(np.uint64).sum()) / L.size + 0.5)


def contrast(im, f):
    return blend(np.uint8(contrast_mean(im)), im, f)


def saturation(im, f):
    return blend(luma(im)[..., None], im, f)


def rgb_to_hsv(a):
    r, g, b = (a[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(F32)
    s = cr / np.where(grey, 1, mx).astype(F32)
    rc, gc, bc = ((mx - x).astype(F32) / cr for x in (r, g, b))
    h = np.where(r == mx, bc - gc,                                                            # fp32
                 np.where(g == mx, (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32),       # double, rounded to fp32
                          (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32)))
    h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
    H = np.clip((h.astype(F64) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((s.astype(F64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, H), np.where(grey, 0, S), mx], -1)
    return out.astype(np.uint8)


def _round_half_away(x):
    """C's round() of non-negative doubles, clipped to 8 bits"""
    fl = np.floor(x)
    return np.clip(fl + (x - fl >= 0.5), 0, 255).astype(np.uint8)


def hsv_to_rgb(a):
    H, S, V = (a[..., i] for i in range(3))
    h6 = H.astype(F64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(F32)
    fs = (S.astype(F64) / 255.0).astype(F32)
    v = V.astype(F64)
    p = _round_half_away(v * (1.0 - fs.astype(F64)))
    q = _round_half_away(v * (1.0 - (fs * f).astype(F64)))                                    # fs * f is a product of two floats: fp32
    t = _round_half_away(v * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64))))
    sel = i.astype(np.int64) % 6
    table = ((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q))
    out = np.empty(a.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.where(S == 0, V, np.choose(sel, [row[c] for row in table]))
    return out


def hue(im, shift):
    hsv = rgb_to_hsv(im)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) % 256
    return hsv_to_rgb(hsv)


def jitter(frame, params):
    """the chain on one uint8 [H, W, 3] frame"""
    if params is None:
        return np.array(frame, dtype=np.uint8)
    order, b, c, s, shift = params
    ops = (lambda im: brightness(im, b), lambda im: contrast(im, c), lambda im: saturation(im, s), lambda im: hue(im, shift))
    im = np.asarray(frame, dtype=np.uint8)
    for o in order:
        im = ops[o](im)
    return im


# ------------------------------------------------------------------------------------------------------------------ cases
ORDERS = list(itertools.permutations(range(4)))          # 24


def all_colours():
    """every RGB triple once, as a 4096 x 4096 frame"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def shift_of(h):
    return int(h * 255) % 256


def order_params(seed=0):
    """one set per permutation; factors drawn, but sample 0 at the low and sample 23 at the high end of monodepth2's ranges"""
    rng = np.random.RandomState(seed)
    out = []
    for i, order in enumerate(ORDERS):
        b, c, s = rng.uniform(0.8, 1.2, 3)
        h = rng.uniform(-0.1, 0.1)
        if i == 0:
            b, c, s, h = 0.8, 0.8, 0.8, -0.1
        if i == len(ORDERS) - 1:
            b, c, s, h = 1.2, 1.2, 1.2, 0.1
        out.append((order, float(b), float(c), float(s), shift_of(h)))
    return out


def random_frames(shape, seed):
    """uint8 frames with structure (a smooth ramp plus noise, some saturated patches) so that every clip and branch is met"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=tuple(shape) + (3,)).astype(np.uint8)
    flat = a.reshape(-1, 3)
    n = flat.shape[0]
    flat[rng.randint(0, n, max(1, n // 16))] = 0                      # black pixels: max == 0
    flat[rng.randint(0, n, max(1, n // 16))] = 255
    k = rng.randint(0, n, max(1, n // 8))
    flat[k] = flat[k][:, :1]                                          # grey pixels
    return a


def degenerate_frames(H, W):
    """black, white, one constant colour (its contrast mean is its own luma), one pure primary"""
    return [np.full((H, W, 3), c, dtype=np.uint8) for c in ((0, 0, 0), (255, 255, 255), (12, 200, 77), (0, 0, 255))]


def random_params(n, seed, prob=0.5):
    """n draws the way the loaders make them (about half of them None)"""
    import supervised_dispnet_amd.data as D
    rng = np.random.RandomState(seed)
    return [D.draw_colour_jitter(rng, prob=prob) for _ in range(n)]
