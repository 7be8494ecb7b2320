#!/usr/bin/env python3
"""What does the device chain of run_inference.py buy?  Fabricates 64 in-memory KITTI-sized frames (375 x 1242 x 3 uint8), a freshly
initialised Disp_vgg_BN at 128 x 416, and reports as one JSON line:

  host_img_s             the reference's per-image chain (--host-chain: numpy / PIL resize, batch-1 forward, colouring and contrast on the host)
  device_img_s           {batch: repeats} of the device chain (dn_imresize_u8, one forward per batch, dn_colorize_u8, dn_contrast_u8, copy back)
  kernel_us_per_image    {batch: {resize, colorize_disp, contrast, colorize_depth, sum}} of the kernels on resident data (HIP events)

Neither chain includes reading or writing files.  Every measurement is a child process of its own under a time limit; the first one that
fails ends the run.

usage: python tools/inference_bench.py [--samples 64] [--repeats 3] [--timeout 300]"""
import argparse, json, pathlib, subprocess, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
ap.add_argument("--step", default=None, help="(internal) host | device:B | kernels:B")
a = ap.parse_args()
BATCHES = (1, 8, 32)

if a.step is None:
    out = {"samples": a.samples, "network": "Disp_vgg_BN 128x416", "frame": [375, 1242], "device_img_s": {}, "kernel_us_per_image": {}}
    for step in ["host"] + ["device:%d" % b for b in BATCHES] + ["kernels:%d" % b for b in BATCHES]:
        cmd = [sys.executable, __file__, "--step", step, "--samples", str(a.samples), "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, text=True)     # a fresh process per step; raises on a time-out
        if p.returncode != 0:
            raise SystemExit("%s failed with status %d" % (step, p.returncode))
        val = json.loads(p.stdout.strip().splitlines()[-1])
        kind, _, b = step.partition(":")
        if kind == "host":
            out["host_img_s"] = val
        else:
            out["device_img_s" if kind == "device" else "kernel_us_per_image"][b] = val
    print(json.dumps(out))
    sys.exit(0)

import numpy as np
import torch
import __graft_entry__
__graft_entry__.build(only_library=True)
import bench
import supervised_dispnet_amd.models as models
from supervised_dispnet_amd import inference
from supervised_dispnet_amd.data import normalization

dev = torch.device("cuda:0")
kind, _, B = a.step.partition(":")
B = int(B or 1)
H, W, h, w = 375, 1242, 128, 416
r = np.random.RandomState(0)
args = inference.build_parser().parse_args(["--network", "disp_vgg_BN", "--pretrained", "none", "--output-disp", "--output-depth"])
mean, std = normalization(False, False)
torch.manual_seed(0)
net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
bench._quiet_init(net)
net.to(dev).eval()
ops = inference.ImageOps(dev)


def rate(fn, n):
    fn()                                   # warm-up pass
    vals = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        vals.append(n / (time.perf_counter() - t0))
    return vals


def host_one(frame):
    output = inference.forward(args, net, inference.host_preprocess(args, frame, mean, std).to(dev))
    return inference.host_images(args, output.cpu())


def device_batch(frames):
    _, img = ops.imresize(frames, (h, w), mean, std)
    return inference.device_images(args, ops, inference.forward(args, net, img))


with torch.no_grad():
    if kind == "host":
        frames = [r.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(a.samples)]
        print(json.dumps(rate(lambda: [host_one(f) for f in frames], len(frames))))
    elif kind == "device":
        frames = [r.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(a.samples)]
        print(json.dumps(rate(lambda: [device_batch(frames[j:j + B]) for j in range(0, len(frames), B)], len(frames))))
    else:
        import ctypes
        st = torch.cuda.current_stream().cuda_stream
        frames = torch.from_numpy(r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
        hw = torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev)
        off = torch.arange(B, dtype=torch.int64, device=dev) * (H * W * 3)
        tx, ty = inference.table_rows(W, w), inference.table_rows(H, h)
        pool = torch.from_numpy(np.concatenate([tx.reshape(-1), ty.reshape(-1)])).to(dev)
        idx = torch.tensor([[0, tx.shape[1] - 2, tx.size, ty.shape[1] - 2]] * B, dtype=torch.int32, device=dev)
        minmax = torch.empty(B * inference.IMAGE_CHUNKS * 2, dtype=torch.int32, device=dev)
        img = torch.empty((B, 3, h, w), device=dev)
        mean_h, std_h = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        disp = torch.rand((B, h, w), device=dev) + 0.01
        rect = inference.garg_rectangle(h, w)
        coloured = ops.colorize(disp, rect)
        steps = {
            "resize": lambda: inference._lib.call("dn_imresize_u8", frames.data_ptr(), hw.data_ptr(), off.data_ptr(), B, h, w, pool.data_ptr(),
                                                  idx.data_ptr(), max(tx.shape[1], ty.shape[1]) - 2, minmax.data_ptr(), None, mean_h, std_h,
                                                  img.data_ptr(), st),
            "colorize_disp": lambda: ops.colorize(disp, rect),
            "contrast": lambda: ops.contrast(coloured, inference.CONTRAST),
            "colorize_depth": lambda: ops.colorize(disp, None, inference.DEPTH_MAX, None, reciprocal=True),
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

        val = {k: timed(fn) for k, fn in steps.items()}
        val["sum"] = sum(val.values())
        print(json.dumps(val))
