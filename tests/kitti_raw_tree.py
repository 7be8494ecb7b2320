"""A tiny KITTI raw tree written by formula (no dataset file): 2 dates x 2 drives, cameras 02 and 03, 6-8 frames of 40 x 120 PNG, oxts
packets whose speeds make the speed rule skip frames (one drive keeps fewer than 3, so its folders are removed), calibration files
written with '%.6e', and velodyne clouds of a few thousand points.  tests/golden/make_kitti_prep_goldens.py runs the reference's
KittiRawLoader on it; the tests run prepare_train_data.py and tests/velo_depth.py on the same tree.

2011_09_28_drive_0002 is one of the reference's test scenes: the golden run holds it out, and the tests pass HELD_OUT to --test-scenes."""
import os

import numpy as np

H0, W0 = 40, 120
DRIVES = [("2011_09_26", "0801", 8), ("2011_09_26", "0802", 6), ("2011_09_28", "0801", 7), ("2011_09_28", "0002", 6)]
HELD_OUT = ["2011_09_28_drive_0002"]
# forward speed per frame: cumulated, a frame is taken when the norm exceeds 2 (and the sum restarts)
SPEEDS = {"0801": [0.8, 0.9, 2.5, 0.3, 0.5, 1.4, 3.0, 0.1], "0802": [0.2, 0.3, 0.4, 0.5, 0.9, 0.1], "0002": [3.0] * 6}
STATIC = [("2011_09_26", "0801", 2), ("2011_09_26", "0801", 5), ("2011_09_28", "0801", 0)]
N_POINTS = 3000

R_RECT = [9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03, 7.402527e-03, 4.351614e-03, 9.999631e-01]
VELO_R = [7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03, 1.480755e-02]
VELO_T = [-4.069766e-03, -7.631618e-02, -2.717806e-01]
IMU_R = [9.999976e-01, 7.553071e-04, -2.035826e-03, -7.854027e-04, 9.998898e-01, -1.482298e-02, 2.024406e-03, 1.482454e-02, 9.998881e-01]
IMU_T = [-8.086759e-01, 3.195559e-01, -7.997231e-01]


def p_rect(cam, date):
    """A 3 x 4 projection for 40 x 120 frames (focal 70, principal point near the centre), a little different per camera and date."""
    f = 70.0 + (1.5 if date.endswith("28") else 0.0)
    bx = {"02": 4.4, "03": -33.0}[cam]
    return [f, 0, 60.3, bx, 0, f, 19.6, 0.21, 0, 0, 1, 2.7e-03]


def drive_name(date, drive):
    return "{}_drive_{}_sync".format(date, drive)


def cloud(date, drive, n, count=N_POINTS):
    """fp32 [count, 4]: forward (some behind the camera), left, up, reflectance."""
    r = np.random.RandomState(1000 * int(drive) + 10 * n + int(date[-2:]))
    u = r.rand(count, 4)
    velo = np.zeros((count, 4), dtype=np.float32)
    velo[:, 0] = (-2 + 40 * u[:, 0] ** 2).astype(np.float32)
    velo[:, 1] = (-12 + 24 * u[:, 1]).astype(np.float32)
    velo[:, 2] = (-2.0 + 3.0 * u[:, 2]).astype(np.float32)
    velo[:, 3] = u[:, 3].astype(np.float32)
    return velo


def frame(date, drive, cam, n, H=H0, W=W0):
    """uint8 [H, W, 3]: smooth waves plus noise, not spanning 0 ... 255 (a byte-scale applied by mistake would show)."""
    r = np.random.RandomState(7 + 1000 * int(drive) + 10 * n + int(cam) + int(date[-2:]))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([120 + 70 * np.sin(x / (9.0 + c) + n) * np.cos(y / (5.0 + c) + int(cam)) for c in range(3)], axis=2)
    return np.clip(img + r.normal(0, 8, (H, W, 3)), 20, 235).astype(np.uint8)


def oxts_packet(drive, n):
    v = np.zeros(30)
    v[0] = 49.0 + 1e-5 * n + 1e-3 * int(drive[-1])       # lat
    v[1] = 8.4 + 2e-5 * n                                # lon
    v[2] = 112.0 + 0.05 * n                              # alt
    v[3], v[4], v[5] = 0.01 * n, -0.02 + 0.004 * n, 0.3 + 0.05 * n   # roll, pitch, yaw
    v[8], v[9], v[10] = SPEEDS[drive][n], 0.05 * n, -0.02             # vf, vl, vu
    return v


def _line(key, values):
    return "{}: {}\n".format(key, " ".join("%.6e" % v for v in values))


def write_tree(root):
    """Write the tree under root (a path) -> root as str."""
    from PIL import Image
    root = str(root)
    for date in sorted(set(d for d, _, _ in DRIVES)):
        folder = os.path.join(root, date)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, "calib_cam_to_cam.txt"), "w") as f:
            f.write("calib_time: 09-Jan-2012 13:57:47\n" + _line("corner_dist", [9.95e-02]) + _line("R_rect_00", R_RECT) +
                    _line("P_rect_02", p_rect("02", date)) + _line("P_rect_03", p_rect("03", date)))
        with open(os.path.join(folder, "calib_velo_to_cam.txt"), "w") as f:
            f.write("calib_time: 15-Mar-2012 11:37:16\n" + _line("R", VELO_R) + _line("T", VELO_T))
        with open(os.path.join(folder, "calib_imu_to_velo.txt"), "w") as f:
            f.write("calib_time: 25-May-2012 16:47:16\n" + _line("R", IMU_R) + _line("T", IMU_T))
    for date, drive, count in DRIVES:
        base = os.path.join(root, date, drive_name(date, drive))
        for sub in ("image_02/data", "image_03/data", "oxts/data", "velodyne_points/data"):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        for n in range(count):
            name = "%010d" % n
            for cam in ("02", "03"):
                Image.fromarray(frame(date, drive, cam, n)).save(os.path.join(base, "image_" + cam, "data", name + ".png"))
            with open(os.path.join(base, "oxts", "data", name + ".txt"), "w") as f:
                f.write(" ".join("%.12e" % v for v in oxts_packet(drive, n)) + "\n")
            cloud(date, drive, n).tofile(os.path.join(base, "velodyne_points", "data", name + ".bin"))
    return root


def write_static_frames(path):
    with open(str(path), "w") as f:
        for date, drive, n in STATIC:
            f.write("{} {} {:010d}\n".format(date, drive_name(date, drive), n))
    return str(path)


def write_test_scenes(path):
    with open(str(path), "w") as f:
        for name in HELD_OUT:
            f.write(name + "\n")
    return str(path)
