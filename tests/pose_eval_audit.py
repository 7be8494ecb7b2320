"""Audit of the pose-evaluation metrics (supervised_dispnet_amd/pose_eval.py: sfm_metric, mono2_metric; csrc/dn_poseeval.hip:
dn_pose_eval_sfm, dn_pose_eval_mono2): an extended-precision restatement, the cases and the error bounds.  A plain module, importable
without a GPU and not collected; tests/test_pose_eval_host.py holds the numpy fp64 chain to it, tests/test_gpu_pose_eval.py the kernels.

The restatement evaluates both contracts in numpy.longdouble (64-bit significand here: its own error is 2^-11 of
fp64's and sits inside the 1.01 below), starting from the same fp32 pose vectors and fp64 ground truth.

The bound.  Every output is a short chain of fp64 operations; an fp64 evaluation of it -- numpy's or the kernel's, in whatever order
they sum -- differs from the exact value by at most

        (operations on the path) x u x (sum of the absolute terms entering the output),   u = 2^-53,

to first order.  That product is accumulated here operation by operation instead of being estimated once: class V carries a value
together with the bound of its error, and each operation adds u x |result| to what its inputs hand on through the operation's
partial derivatives (a sum of n products adds n x u x sum|a_i b_i|, which holds for any summation order and with or without fused
multiply-adds: numpy's matmul / pairwise sums and the kernel's index-order sums are both covered).  So the longest path contributes
exactly its operation count times u times the absolute terms, and shorter paths contribute less.  At the end: x 1.01 for the higher
orders.  A 3 x 3 inverse X of A carries |X| E_A |X| + INV_OPS x u x |X| |A| |X| (entrywise), INV_OPS = 27: numpy inverts by LU with two
triangular solves (3 stages of at most 3 n = 9 operations on a path), the kernel by cofactors (8 on its longest path); rotations are
perfectly conditioned, so there is no pivot growth to add.  |(r_1 .. r_n)|_2 carries |(e_1 .. e_n)|_2 + (n + 2 + SQRT) x u x its value
(it stays sharp where the residual is tiny, which sqrt of a separately bounded sum of squares does not).

Library functions: an fp64 sin / cos / atan2 / sqrt call adds its own error, ULP[f] units in the last place of its result.  The ROCm
device-library documentation with the table of these errors is NOT part of this ROCm install (nothing under its share / doc trees
states one), so by the rule of the audit the figures are the errors measured against longdouble on the CPU for numpy's own functions
(measure_ulps(): sin 0.52, cos 0.52, atan2 0.78, sqrt 0.50 ulp over 6e5 arguments each), times two.  test_pose_eval_host.py measures
them again and checks that they are inside ULP.

Measured (the tests print every figure): the worst share of a bound is 0.119 on an MI355X (RE, a reference frame turned by pi, N 65,
L 3) and 0.091 for numpy fp64 on the CPU (the same case); MEASURED at the end of this file, DESIGN.md section 21.
"""
import functools

import numpy as np

LD = np.longdouble
U = LD(2) ** -53
HIGHER_ORDERS = LD("1.01")
INV_OPS = 27
ULP = {"sin": 1.04, "cos": 1.04, "atan2": 1.56, "sqrt": 1.0}      # 2 x measured (see the docstring); one ulp = 2 u


def measure_ulps(n=600000, seed=0):
    """The largest error, in units in the last place of the result, of numpy's fp64 sin / cos / arctan2 / sqrt against longdouble."""
    rng = np.random.RandomState(seed)

    def worst(f, *args):
        got, ref = f(*args), f(*[a.astype(LD) for a in args])
        return float(np.max(np.abs(got.astype(LD) - ref) / np.spacing(np.abs(got)).astype(LD)))

    x = np.concatenate([rng.uniform(-10, 10, n * 2 // 3), rng.uniform(-1e-3, 1e-3, n // 6),
                        (rng.standard_normal(n // 6).astype(np.float32) * 3).astype(np.float64)])
    y, xx = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    return {"sin": worst(np.sin, x), "cos": worst(np.cos, x), "atan2": max(worst(np.arctan2, y, xx), worst(np.arctan2, np.abs(y) * 1e-9, xx)),
            "sqrt": worst(np.sqrt, np.abs(x))}


# ------------------------------------------------------------------------------------------------ values with error bounds
class V(object):
    """A longdouble array `v` and the first-order bound `e` of the absolute error an fp64 evaluation has accumulated in it."""

    def __init__(self, v, e=0):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.broadcast_to(np.asarray(e, dtype=LD), self.v.shape)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def __neg__(self):
        return V(-self.v, self.e)

    def __add__(self, o):
        o = _v(o)
        v = self.v + o.v
        return V(v, self.e + o.e + U * np.abs(v))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-_v(o))

    def __rsub__(self, o):
        return _v(o) + (-self)

    def __mul__(self, o):
        o = _v(o)
        v = self.v * o.v
        return V(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _v(o)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = self.v / o.v
            return V(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + U * np.abs(v))


def _v(x):
    return x if isinstance(x, V) else V(x)


def exact(x):
    return V(np.asarray(x, dtype=np.float64).astype(LD))


def _lib_call(name, v, e_in):
    return V(v, e_in + 2 * ULP[name] * U * np.abs(v))


def vsin(a):
    return _lib_call("sin", np.sin(a.v), a.e)


def vcos(a):
    return _lib_call("cos", np.cos(a.v), a.e)


def vatan2(y, x):
    r2 = x.v * x.v + y.v * y.v
    with np.errstate(invalid="ignore", divide="ignore"):
        return _lib_call("atan2", np.arctan2(y.v, x.v), (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / r2)


def dot(a, b):
    """sum_i a_i b_i of n terms in any order: n x u x sum |a_i b_i| on top of what the inputs carry."""
    n = len(a)
    v = sum(x.v * y.v for x, y in zip(a, b))
    mag = sum(np.abs(x.v * y.v) for x, y in zip(a, b))
    return V(v, sum(np.abs(x.v) * y.e + np.abs(y.v) * x.e for x, y in zip(a, b)) + n * U * mag)


def norm2(r):
    n = len(r)
    v = np.sqrt(sum(x.v * x.v for x in r))
    return V(v, np.sqrt(sum(x.e * x.e for x in r)) + (n + 2 + 2 * ULP["sqrt"]) * U * v)


def matmul3(A, B):
    return [[dot(A[i], [B[k][j] for k in range(3)]) for j in range(3)] for i in range(3)]


def matvec_add(A, x, t):
    """A x + t as one 4-term sum per row (numpy: a matmul and an add, or a 4 x 4 product with the unit entry; the kernel: 3 + 1)."""
    one = V(np.ones_like(t[0].v))
    return [dot(list(A[i]) + [one], list(x) + [t[i]]) for i in range(3)]


def inv3(A):
    a = [[A[i][j].v for j in range(3)] for i in range(3)]
    c = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3] for j in range(3)]
         for i in range(3)]
    det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2]
    X = [[c[j][i] / det for j in range(3)] for i in range(3)]
    aX = [[np.abs(X[i][j]) for j in range(3)] for i in range(3)]

    def sandwich(M):
        return [[sum(aX[i][k] * M[k][l] * aX[l][j] for k in range(3) for l in range(3)) for j in range(3)] for i in range(3)]

    eA = sandwich([[A[i][j].e for j in range(3)] for i in range(3)])
    rA = sandwich([[np.abs(a[i][j]) for j in range(3)] for i in range(3)])
    return [[V(X[i][j], eA[i][j] + INV_OPS * U * rA[i][j]) for j in range(3)] for i in range(3)]


def bound(x):
    return x.e * HIGHER_ORDERS


# ------------------------------------------------------------------------------------------------ the two contracts
def _pose_matrix(vec, rotation_mode):
    """fp32 [N, 6] -> (rotation 3 x 3 of V [N], translation 3 of V [N])."""
    v = np.asarray(vec, dtype=np.float32).astype(np.float64)
    t = [exact(v[:, i]) for i in range(3)]
    x, y, z = exact(v[:, 3]), exact(v[:, 4]), exact(v[:, 5])
    zero, one = V(np.zeros(len(v))), V(np.ones(len(v)))
    if rotation_mode == "euler":
        cx, sx, cy, sy, cz, sz = vcos(x), vsin(x), vcos(y), vsin(y), vcos(z), vsin(z)
        zm = [[cz, -sz, zero], [sz, cz, zero], [zero, zero, one]]
        ym = [[cy, zero, sy], [zero, one, zero], [-sy, zero, cy]]
        xm = [[one, zero, zero], [zero, cx, -sx], [zero, sx, cx]]
        return matmul3(matmul3(xm, ym), zm), t
    q = [one, x, y, z]
    nrm = norm2(q)
    nrm = V(nrm.v, nrm.e + 2 * U * nrm.v)                  # (the four squares summed as a 4-term sum)
    w, x, y, z = one / nrm, x / nrm, y / nrm, z / nrm
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return [[w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz],
            [2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx],
            [2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2]], t


def _scaled_residual_norm(g, p, points):
    """s = sum(g p) / sum(p p); |g - s p|_2 / points on lists of V."""
    s = dot(g, p) / dot(p, p)
    return norm2([a - s * b for a, b in zip(g, p)]) / points


def sfm(pose, gt, rotation_mode="euler"):
    """pose fp32 [N, L-1, 6], gt fp64 [N, L, 3, 4] -> (values longdouble [N, 2], bounds longdouble [N, 2])."""
    pose = np.asarray(pose, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float64)
    N, L = gt.shape[0], gt.shape[1]
    P = np.concatenate([pose[:, :L // 2], np.zeros((N, 1, 6), np.float32), pose[:, L // 2:]], axis=1)
    R0, t0 = _pose_matrix(P[:, 0], rotation_mode)
    g_t, p_t, re = [], [], V(np.zeros(N))
    for k in range(L):
        Mr, Mt = _pose_matrix(P[:, k], rotation_mode)
        Rk = inv3(Mr)
        tk = [-dot(Rk[i], Mt) for i in range(3)]
        Fr = matmul3(R0, Rk)
        Ft = matvec_add(R0, tk, t0)
        g_t += [exact(gt[:, k, i, 3]) for i in range(3)]
        p_t += Ft
        G = [[exact(gt[:, k, i, j]) for j in range(3)] for i in range(3)]
        D = matmul3(G, inv3(Fr))
        s = norm2([D[0][1] - D[1][0], D[1][2] - D[2][1], D[0][2] - D[2][0]])
        c = (D[0][0] + D[1][1] + D[2][2]) - 1
        re = re + vatan2(s, c)
    ate = _scaled_residual_norm(g_t, p_t, L)
    re = re / L
    return np.stack([ate.v, re.v], 1), np.stack([bound(ate), bound(re)], 1)


def _transform(pose):
    """fp32 [P, 6] (axisangle, translation) -> (Rodrigues rotation 3 x 3 of V [P], translation 3 of V [P])."""
    v = np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(-1, 6)
    a = [exact(v[:, i]) for i in range(3)]
    t = [exact(v[:, 3 + i]) for i in range(3)]
    angle = norm2(a)
    dn = angle + 1e-7
    x, y, z = a[0] / dn, a[1] / dn, a[2] / dn
    ca, sa = vcos(angle), vsin(angle)
    C = 1 - ca
    xs, ys, zs, xC, yC, zC = x * sa, y * sa, z * sa, x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    return [[x * xC + ca, xyC - zs, zxC + ys], [xyC + zs, y * yC + ca, yzC - xs], [zxC - ys, yzC + xs, z * zC + ca]], t


def mono2(pose, Q, track=5):
    """pose fp32 [P, 6], Q fp64 [P, 4, 4] -> (values longdouble [P], bounds longdouble [P])."""
    Tr, Tt = _transform(pose)
    Q = np.asarray(Q, dtype=np.float64)
    P = Q.shape[0]
    vals, bnds = np.zeros(P, LD), np.zeros(P, LD)
    eye = [[V(LD(1.0 if i == j else 0.0)) for j in range(3)] for i in range(3)]
    for i in range(P):
        last = min(i + track - 1, P)
        Cr, Ct, Gr, Gt = eye, [V(LD(0))] * 3, eye, [V(LD(0))] * 3
        g, p = [V(LD(0))] * 3, [V(LD(0))] * 3            # point 0 of both trajectories; the offset gt_0 - pred_0 is exactly 0
        for j in range(i, last):
            tr = [[Tr[a][b][j] for b in range(3)] for a in range(3)]
            Ct = matvec_add(Cr, [Tt[a][j] for a in range(3)], Ct)
            Cr = matmul3(Cr, tr)
            Gt = matvec_add(Gr, [exact(Q[j, a, 3]) for a in range(3)], Gt)
            Gr = matmul3(Gr, [[exact(Q[j, a, b]) for b in range(3)] for a in range(3)])
            g, p = g + Gt, p + Ct
        r = _scaled_residual_norm(g, p, last - i + 1)
        vals[i], bnds[i] = r.v, bound(r)
    return vals, bnds


# ------------------------------------------------------------------------------------------------ cases
def _rng(tag):
    return np.random.RandomState(sum((i + 1) * ord(c) for i, c in enumerate(tag)) % (2 ** 31))


def _euler(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


def trajectory(rng, n, turn=0.05, step=1.0):
    """fp64 [n, 3, 4]: a drive of about `step` per frame that turns by about `turn` rad per frame."""
    out = np.zeros((n, 3, 4))
    ang, pos = rng.uniform(-0.3, 0.3, 3), rng.uniform(-5, 5, 3)
    for k in range(n):
        out[k, :, :3], out[k, :, 3] = _euler(*ang), pos
        ang = ang + rng.uniform(-turn, turn, 3) + [0, turn, 0]
        pos = pos + out[k, :, :3] @ (np.array([0.05, 0.02, 1.0]) * step + rng.uniform(-0.05, 0.05, 3) * step)
    return out


def _to44(m):
    out = np.zeros((4, 4))
    out[:3], out[3, 3] = m, 1
    return out


def _euler_angles(R):
    return np.array([np.arctan2(-R[1, 2], R[2, 2]), np.arcsin(np.clip(R[0, 2], -1, 1)), np.arctan2(-R[0, 1], R[0, 0])])


def _quat_vector(R):
    w = np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4 * w) / w


def _axisangle(R):
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    nrm = np.linalg.norm(ax)
    return ax / nrm * ang if nrm > 1e-12 else np.zeros(3)


def _compensate(p):
    p = p.copy()
    first = p[0].copy()
    p[:, :, -1] -= first[:, -1]
    return np.linalg.inv(first[:, :3]) @ p


SFM_KINDS = ("well", "tiny", "zeros", "identity_rot", "pi", "beyond_pi", "quat_unnormalised")
SFM_SIZES = ((1, 3), (2, 5), (65, 3), (257, 5))
MONO2_KINDS = ("well", "tiny", "zeros", "pi", "beyond_pi")
MONO2_SIZES = (1, 3, 4, 5, 70)


@functools.lru_cache(maxsize=None)
def sfm_case(kind, N, L):
    """-> (pose fp32 [N, L-1, 6], gt fp64 [N, L, 3, 4], rotation mode)."""
    rng = _rng("sfm:%s:%d:%d" % (kind, N, L))
    mode = "quat" if kind == "quat_unnormalised" or (kind == "well" and L == 5) else "euler"
    traj = trajectory(rng, N + L - 1)
    gt = np.stack([_compensate(traj[n:n + L]) for n in range(N)])
    scale = 1e6 if kind == "tiny" else 7.0
    pose = np.zeros((N, L - 1, 6))
    mid = L // 2
    for n in range(N):
        G = [_to44(g) for g in gt[n]]
        for g in G:
            g[:3, 3] /= scale
        for j, k in enumerate([k for k in range(L) if k != mid]):
            M = np.linalg.inv(G[k]) @ G[mid]               # F_k = M_0 inv(M_k) = G_k with M_mid = I
            pose[n, j, :3] = M[:3, 3] * (1 + rng.uniform(-0.05, 0.05, 3))
            pose[n, j, 3:] = (_quat_vector(M[:3, :3]) if mode == "quat" else _euler_angles(M[:3, :3])) + rng.uniform(-0.01, 0.01, 3)
    if kind == "zeros":                                     # every other snippet predicts no motion at all: 0 / 0
        pose[::2, :, :3] = 0
    elif kind == "identity_rot":                            # no rotation anywhere, predicted or true: RE is exactly 0
        pose[:, :, 3:] = 0
        gt[:, :, :, :3] = np.eye(3)
    elif kind == "pi":                                      # the last reference is turned by pi about x, y or z
        pose[:, -1, 3:] = 0
        pose[np.arange(N), -1, 3 + np.arange(N) % 3] = np.pi
    elif kind == "beyond_pi":
        pose[:, :, 3:] += rng.choice([-7.0, -5.5, 4.0, 6.5, 9.0], size=(N, L - 1, 3))
    elif kind == "quat_unnormalised":
        pose[:, :, 3:] = rng.uniform(-3, 3, (N, L - 1, 3))
    return pose.astype(np.float32), gt, mode


@functools.lru_cache(maxsize=None)
def mono2_case(kind, P):
    """-> (pose fp32 [P, 6], Q fp64 [P, 4, 4])."""
    rng = _rng("mono2:%s:%d" % (kind, P))
    traj = trajectory(rng, P + 1)
    G = [_to44(g) for g in traj]
    Q = np.array([np.linalg.inv(np.linalg.inv(G[i]) @ G[i + 1]) for i in range(P)]).reshape(P, 4, 4)
    scale = 1e6 if kind == "tiny" else 30.0
    pose = np.zeros((P, 6))
    for i in range(P):
        pose[i, :3] = _axisangle(Q[i, :3, :3]) + rng.uniform(-0.005, 0.005, 3)
        pose[i, 3:] = Q[i, :3, 3] / scale * (1 + rng.uniform(-0.05, 0.05, 3))
    if kind == "zeros":                                     # the windows from P // 2 on hold only pairs that predict no motion: 0 / 0
        pose[P // 2:, 3:] = 0
    elif kind == "pi":
        ax = rng.standard_normal((P, 3))
        pose[:, :3] = ax / np.linalg.norm(ax, axis=1, keepdims=True) * np.pi
    elif kind == "beyond_pi":
        ax = rng.standard_normal((P, 3))
        pose[:, :3] = ax / np.linalg.norm(ax, axis=1, keepdims=True) * rng.choice([4.0, 5.5, 7.0, 9.5], size=(P, 1))
    if kind != "zeros" and P > 2:
        pose[1, :3] = 0                                     # a zero axis-angle: 0 / (0 + 1e-7)
    return pose.astype(np.float32), Q


def sfm_cases():
    return [(kind, N, L) for kind in SFM_KINDS for (N, L) in SFM_SIZES]


def mono2_cases():
    return [(kind, P) for kind in MONO2_KINDS for P in MONO2_SIZES]


@functools.lru_cache(maxsize=None)
def sfm_reference(kind, N, L):
    pose, gt, mode = sfm_case(kind, N, L)
    return sfm(pose, gt, mode)


@functools.lru_cache(maxsize=None)
def mono2_reference(kind, P):
    return mono2(*mono2_case(kind, P))


def share(got, ref, bnd):
    """The largest |got - ref| / bound over the finite references (0 where the bound is 0 and the values agree), after checking that
    got is NaN exactly where the reference is."""
    got, ref, bnd = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bnd, dtype=LD)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs: got %s, reference %s" % (np.isnan(got).sum(), nan.sum())
    err = np.abs(got - ref)[~nan]
    b = bnd[~nan]
    if err.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(err == 0, 0, err / b)
    return float(np.max(s))


# Worst |got - reference| / bound over all cases, as printed by the tests (a share of 1 would be the bound itself):
#   numpy fp64 on the CPU:      sfm ATE 0.022, RE 0.091 (pi, N 65, L 3); mono2 0.0097
#   the kernels on an MI355X:   sfm ATE 0.022, RE 0.119 (pi, N 65, L 3); mono2 0.0115 (tiny, P 5)
#   kernels against numpy fp64: sfm ATE 0.028, RE 0.109; mono2 0.0126
MEASURED = {"numpy": {"sfm_ate": 0.022, "sfm_re": 0.091, "mono2": 0.0097},
            "mi355x": {"sfm_ate": 0.022, "sfm_re": 0.119, "mono2": 0.0115}}
