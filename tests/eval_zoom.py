"""numpy restatement of the number contract of the device zoom (dn_zoom3_prefilter + dn_zoom3_clip):
scipy.ndimage.zoom(a, (H/h, W/w)) with scipy's defaults (order 3, mode 'constant', cval 0, prefilter, grid_mode=False) on a float32
plane.  tests/test_eval_device_host.py pins it to scipy bit for bit; the GPU tests compare the kernels with scipy directly."""
import numpy as np

# the seven (network resolution -> ground-truth size) pairs the zoom is checked on: the four KITTI sizes at 128x416, NYU, the
# monodepth2 resolution, and one small odd pair
SHAPE_PAIRS = [((128, 416), (375, 1242)), ((128, 416), (370, 1226)), ((128, 416), (376, 1241)), ((128, 416), (374, 1238)),
               ((256, 352), (480, 640)), ((192, 640), (375, 1242)), ((40, 56), (97, 131))]


def smooth_positive_map(h, w, seed):
    """A depth-like float32 plane: a smooth positive map plus noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = 12.0 + 9.0 * np.sin(y / (0.23 * h) + 0.3) * np.cos(x / (0.17 * w)) + 0.05 * x / w + rng.normal(0.0, 0.4, (h, w))
    return np.maximum(a, 0.05).astype(np.float32)


def axis_taps(n, O):
    """Per output index of one axis: (valid [O] bool, taps [O, 4] mirrored source indices, weights [O, 4] fp64)."""
    o = np.arange(O, dtype=np.float64)
    x = o * (np.float64(n - 1) / np.float64(O - 1)) if O > 1 else np.zeros(1)
    valid = (x >= 0) & (x <= n - 1)
    f = np.floor(x)
    t = x - f
    z = 1.0 - t
    w = np.empty((O, 4))
    w[:, 1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 0] = z * z * z / 6.0
    w[:, 3] = 1.0 - w[:, 0] - w[:, 1] - w[:, 2]
    idx = f.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :]
    period = 2 * (n - 1)
    idx = np.abs(idx) % period
    idx = np.where(idx > n - 1, period - idx, idx)
    return valid, idx, w


def zoom3(a, out_hw):
    """The restatement: float32 [h, w] -> float32 [H, W]."""
    from scipy.ndimage import spline_filter
    h, w = a.shape
    H, W = out_hw
    coef = spline_filter(a, order=3, output=np.float64, mode="mirror")
    vy, iy, wy = axis_taps(h, H)
    vx, ix, wx = axis_taps(w, W)
    acc = np.zeros((H, W))
    for i in range(4):
        for j in range(4):
            acc += coef[iy[:, i][:, None], ix[:, j][None, :]] * (wy[:, i][:, None] * wx[:, j][None, :])
    acc[~vy, :] = 0.0
    acc[:, ~vx] = 0.0
    return acc.astype(np.float32)
