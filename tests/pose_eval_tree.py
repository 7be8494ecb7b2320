"""A tiny synthetic KITTI-odometry tree for the pose evaluation (a plain module: tests/golden/make_pose_eval_goldens.py writes it for the
reference's reader, the tests write it again for ours).  Everything is closed-form: no random numbers, the same bytes everywhere.

    ROOT/sequences/<seq>/image_2/000000.png ...     ROOT/poses/<seq>.txt (12 numbers per row, '%.12e')         write_odometry
    ROOT/<seq>/000000.<ext> ...                     ROOT/<seq>/poses.txt                                       write_folders
"""
import os

import numpy as np

GOLDEN_SEQUENCES = (("09", 7), ("10", 4))      # the golden's tree: two sequences of 7 and 4 frames
GOLDEN_SIZE = (8, 12)
GOLDEN_LENGTHS = (3, 5)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    xm = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ym = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    zm = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return xm @ ym @ zm


def poses(name, n):
    """fp64 [n, 3, 4]: a forward drive with a slow turn; the first pose is neither the identity nor at the origin."""
    phase = 0.37 * (sum(ord(c) for c in name) % 11)
    out = np.zeros((n, 3, 4))
    for k in range(n):
        out[k, :, :3] = _rot(0.03 * np.sin(0.9 * k + phase) + 0.1, 0.07 * k + 0.2 + 0.1 * phase, 0.02 * np.cos(0.5 * k + phase) - 0.05)
        out[k, :, 3] = [3.0 + 0.11 * k * np.sin(0.4 * k + phase), -1.0 + 0.02 * k, 5.0 + 0.8 * k + 0.05 * k * k]
    return out


def frame(name, k, h, w):
    """uint8 [h, w, 3]: a pattern that differs per sequence, frame, pixel and channel and uses the whole byte range."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    base = sum(ord(ch) for ch in name)
    return ((y * 37 + x * 11 + c * 83 + k * 29 + base * 7 + (x * y) % 5 * 17) % 256).astype(np.uint8)


def _write_frames(folder, name, n, h, w, ext):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for k in range(n):
        Image.fromarray(frame(name, k, h, w)).save(os.path.join(folder, "%06d.%s" % (k, ext)))


def write_odometry(root, sequences=GOLDEN_SEQUENCES, size=GOLDEN_SIZE):
    os.makedirs(os.path.join(root, "poses"), exist_ok=True)
    for name, n in sequences:
        _write_frames(os.path.join(root, "sequences", name, "image_2"), name, n, size[0], size[1], "png")
        np.savetxt(os.path.join(root, "poses", name + ".txt"), poses(name, n).reshape(n, 12), fmt="%.12e")
    return root


def write_folders(root, sequences=GOLDEN_SEQUENCES, size=GOLDEN_SIZE, ext="png"):
    for name, n in sequences:
        _write_frames(os.path.join(root, name), name, n, size[0], size[1], ext)
        np.savetxt(os.path.join(root, name, "poses.txt"), poses(name, n).reshape(n, 12), fmt="%.12e")
    return root
