"""numpy restatement of dn_velo_depth's number contract (include/dispnet_hip.h), written from the contract and
independent of supervised_dispnet_amd: the velodyne projection of data/kitti_raw_loader.py:243-300 with every sum in a FIXED order,
and the reference's map: last write wins, then the minimum of every duplicated key at the pixel of the key's first point.
The reference multiplies through BLAS, whose summation order is its own: equality with the reference's maps is a property of the
committed inputs (tests/test_kitti_prep_host.py checks it), equality with the kernel is the contract."""
import numpy as np


def project(points, M, lim_h, lim_w):
    """points fp32 [n, 4], M fp64 [3, 4] -> (index into points, row, col, depth) of the points inside the image, in point order."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 4)
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    idx = np.flatnonzero(points[:, 0] >= 0)                                  # drops NaN too
    x, y, z = (points[idx, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        p = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]
        col = np.round(p[0] / p[2]) - 1
        row = np.round(p[1] / p[2]) - 1
        ok = (col >= 0) & (row >= 0) & (col < lim_w) & (row < lim_h)
    return idx[ok], row[ok].astype(np.int64), col[ok].astype(np.int64), p[2][ok]


def depth_map(points, M, h, w, lim_h=None, lim_w=None):
    """-> fp32 [h, w]."""
    lim_h, lim_w = h if lim_h is None else lim_h, w if lim_w is None else lim_w
    _, row, col, depth = project(points, M, lim_h, lim_w)
    out = np.zeros((h, w), dtype=np.float64)
    for r, c, d in zip(row, col, depth):                                     # last write wins
        out[r, c] = d
    key = row * (w - 1) + col - 1
    groups = {}
    for n, k in enumerate(key):
        groups.setdefault(int(k), []).append(n)
    for members in groups.values():
        if len(members) > 1:
            out[row[members[0]], col[members[0]]] = depth[members].min()
    out[out < 0] = 0
    return out.astype(np.float32)


def depth_maps(clouds, Ms, h, w, lim_h=None, lim_w=None):
    return np.stack([depth_map(c, M, h, w, lim_h, lim_w) for c, M in zip(clouds, Ms)])


def kitti_gt_inputs(mk):
    """The synthetic scene of tests/golden/kitti_gt.npz as dn_velo_depth takes it -> (cloud fp32 [n, 4], P_velo2im fp64 [3, 4]): the
    calibration through the '%.6e' text the golden generator (mk = tests/golden/make_goldens.py as a module) wrote into its calibration
    files, multiplied with the reference's two np.dot calls."""
    p_rect, r_rect, r, t, velo = mk.synthetic_kitti_scene()
    rd = lambda a: np.array([float("%.6e" % v) for v in a])
    r4 = np.eye(4)
    r4[:3, :3] = rd(r_rect).reshape(3, 3)
    velo2cam = np.vstack((np.hstack((rd(r).reshape(3, 3), rd(t)[:, None])), [0, 0, 0, 1.0]))
    return velo.astype(np.float32), np.dot(np.dot(rd(p_rect).reshape(3, 4), r4), velo2cam)


def golden_map(g, shape):
    """tests/golden/kitti_gt.npz's fp64 map of one shape, cast to fp32."""
    want = np.zeros(shape, np.float32)
    yx = g["depth:%dx%d:yx" % shape]
    want[yx[:, 0], yx[:, 1]] = g["depth:%dx%d:val" % shape].astype(np.float32)
    return want
