#!/usr/bin/env python3
"""What does the device chain of prepare_train_data.py buy?  Fabricates in-memory KITTI-sized frames (375 x 1242 uint8) and velodyne
clouds of about 120 k points, and reports as one JSON line:

  host_frames_s          resize (PIL) + depth map (kitti_eval.project_velodyne / scatter_depth_min_duplicates, the host chain) per frame,
                         one thread: three repeats
  device_frames_s        {batch: three repeats} of kitti_prep.device_batch (one upload, dn_resize_u8 + dn_velo_depth, one download) at
                         batch 1 / 8 / 32
  kernel_us_per_frame    {batch: {resize, depth}} of the two entry points on resident data (HIP events)

Neither chain includes PNG decode, reading .bin files, JPEG encode or np.save: those stay on the host in both and
bound the end-to-end rate of the command.  Every measurement is a child process of its own under a time limit; the first one that
fails ends the run.

usage: python tools/prep_bench.py [--frames 64] [--repeats 3] [--timeout 300]"""
import argparse, json, pathlib, subprocess, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
ap.add_argument("--step", default=None, help="(internal) host | device:B | kernels:B")
a = ap.parse_args()
BATCHES = (1, 8, 32)
H, W, h, w, NPTS = 375, 1242, 128, 416, 120000

if a.step is None:
    out = {"frames": a.frames, "frame": [H, W], "points": NPTS, "size": [h, w], "device_frames_s": {}, "kernel_us_per_frame": {}}
    for step in ["host"] + ["device:%d" % b for b in BATCHES] + ["kernels:%d" % b for b in BATCHES]:
        cmd = [sys.executable, __file__, "--step", step, "--frames", str(a.frames), "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, text=True)     # a fresh process per step; raises on a time-out
        if p.returncode != 0:
            raise SystemExit("%s failed with status %d" % (step, p.returncode))
        val = json.loads(p.stdout.strip().splitlines()[-1])
        kind, _, b = step.partition(":")
        if kind == "host":
            out["host_frames_s"] = val
        else:
            out[{"device": "device_frames_s", "kernels": "kernel_us_per_frame"}[kind]][b] = val
    print(json.dumps(out))
    sys.exit(0)

import numpy as np
from supervised_dispnet_amd import kitti_eval as KE, kitti_prep as KP

kind, _, B = a.step.partition(":")
B = int(B or 1)
r = np.random.RandomState(0)
# a KITTI calibration (2011_09_26, camera 02) scaled to 128 x 416
P_RECT = np.array([7.215377e+02, 0, 6.095593e+02, 4.485728e+01, 0, 7.215377e+02, 1.728540e+02, 2.163791e-01, 0, 0, 1, 2.745884e-03]).reshape(3, 4)
R_RECT = np.array([9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03, 7.402527e-03, 4.351614e-03, 9.999631e-01])
RT = np.hstack((np.array([7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03,
                          1.480755e-02]).reshape(3, 3), np.array([[-4.069766e-03], [-7.631618e-02], [-2.717806e-01]])))
P_RECT[0] *= w / W
P_RECT[1] *= h / H
R4 = np.eye(4)
R4[:3, :3] = R_RECT.reshape(3, 3)
M = np.dot(np.dot(P_RECT, R4), np.vstack((RT, [0, 0, 0, 1.0])))


def fabricate(n):
    frames, clouds = [], []
    for _ in range(n):
        frames.append(r.randint(0, 256, (H, W, 3)).astype(np.uint8))
        u = r.rand(NPTS, 4)
        c = np.empty((NPTS, 4), np.float32)
        c[:, 0], c[:, 1], c[:, 2], c[:, 3] = -20 + 100 * u[:, 0] ** 2, -40 + 80 * u[:, 1], -2 + 3 * u[:, 2], u[:, 3]   # a full sweep: ~half behind
        clouds.append(c)
    return frames, clouds


def host_frame(frame, cloud):
    img = KP.host_resize(frame, h, w)
    velo = cloud.copy()
    velo[:, 3] = 1
    pts = KE.project_velodyne(velo, P_RECT, R_RECT, RT, (float(h), float(w)))
    return img, KE.scatter_depth_min_duplicates(pts, (h, w)).astype(np.float32)


def rate(fn, n, sync=lambda: None):
    fn()                                   # warm-up pass
    vals = []
    for _ in range(a.repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        vals.append(n / (time.perf_counter() - t0))
    return vals


if kind == "host":
    frames, clouds = fabricate(a.frames)
    print(json.dumps(rate(lambda: [host_frame(f, c) for f, c in zip(frames, clouds)], len(frames))))
    sys.exit(0)

import torch
import __graft_entry__
__graft_entry__.build(only_library=True)
from supervised_dispnet_amd import _lib, inference

dev = torch.device("cuda:0")
ops = inference.ImageOps(dev)
if kind == "device":
    frames, clouds = fabricate(a.frames)
    Ms = np.stack([M] * B)
    print(json.dumps(rate(lambda: [KP.device_batch(ops, frames[j:j + B], (h, w), clouds[j:j + B], Ms[:len(frames[j:j + B])], (h, w), (h, w))
                                   for j in range(0, len(frames), B)], len(frames), torch.cuda.synchronize)))
else:
    frames, clouds = fabricate(B)
    st = torch.cuda.current_stream().cuda_stream
    _, _, _, flat, hw, off, idx, taps = ops.pack(frames, (h, w))
    d_flat, d_hw, d_off, d_idx = (torch.from_numpy(x).to(dev) for x in (flat, hw, off, idx))
    u8 = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
    pt_off = np.zeros(B + 1, np.int64)
    pt_off[1:] = np.cumsum([len(c) for c in clouds])
    d_pts, d_pt_off, d_M = torch.from_numpy(np.concatenate(clouds)).to(dev), torch.from_numpy(pt_off).to(dev), torch.from_numpy(np.stack([M] * B)).to(dev)
    need = _lib.load().dn_velo_depth_workspace_bytes(B, h, w, int(pt_off[-1]))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    depth = torch.empty((B, h, w), device=dev)
    steps = {
        "resize": lambda: ops.resize_packed(B, h, w, d_flat.data_ptr(), d_hw.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), taps,
                                            u8.data_ptr()),
        "depth": lambda: _lib.call("dn_velo_depth", d_pts.data_ptr(), d_pt_off.data_ptr(), int(pt_off[-1]), d_M.data_ptr(), B, h, w, float(h),
                                   float(w), ws.data_ptr(), need, depth.data_ptr(), st),
    }

    def timed(fn, reps=20):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps / B

    print(json.dumps({k: timed(fn) for k, fn in steps.items()}))
