#!/usr/bin/env python3
"""What does eval_disp.py --eval-batch buy?  Fabricates 64 in-memory KITTI-shaped samples (375 x 1242 frame, ~5 %-dense ground truth,
Garg-crop mask), a freshly initialised Disp_vgg_BN at 128 x 416, and reports as one JSON line:

  host_img_s             the loop of test_disp.evaluate_sample (batch-1 forward, copy back, scipy zoom, numpy metrics): three repeats
  device_img_s           {batch: three repeats} of supervised_dispnet_amd.evaluation.DeviceEvaluator at batch 1 / 8 / 32
  device_resize_img_s    with --device-resize: the same with eval_disp.py --device-resize (raw frames uploaded, dn_imresize_u8), measured
                         right after the run without it, batch by batch
  kernel_us_per_image    {batch: {prefilter, zoom, errors, sum}} of the three new kernels on resident data (HIP events)

Both chains include the resize of the frame (on the host unless --device-resize); neither includes reading files (--readers overlaps that in eval_disp.py).
Every measurement is a child process of its own under a time limit; the first one that fails ends the run.

usage: python tools/eval_chain_bench.py [--samples 64] [--repeats 3] [--timeout 300] [--device-resize]"""
import argparse, json, pathlib, subprocess, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
ap.add_argument("--device-resize", action="store_true", help="also measure the device chain with eval_disp.py --device-resize")
ap.add_argument("--step", default=None, help="(internal) host | device:B | resize:B | kernels:B")
a = ap.parse_args()
BATCHES = (1, 8, 32)

if a.step is None:
    out = {"samples": a.samples, "network": "Disp_vgg_BN 128x416", "gt": [375, 1242], "device_img_s": {}, "kernel_us_per_image": {}}
    if a.device_resize:
        out["device_resize_img_s"] = {}
    pairs = [s for b in BATCHES for s in ["device:%d" % b] + (["resize:%d" % b] if a.device_resize else [])]
    for step in ["host"] + pairs + ["kernels:%d" % b for b in BATCHES]:
        cmd = [sys.executable, __file__, "--step", step, "--samples", str(a.samples), "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, text=True)     # a fresh process per step; raises on a time-out
        if p.returncode != 0:
            raise SystemExit("%s failed with status %d" % (step, p.returncode))
        val = json.loads(p.stdout.strip().splitlines()[-1])
        kind, _, b = step.partition(":")
        if kind == "host":
            out["host_img_s"] = val
        else:
            out[{"device": "device_img_s", "resize": "device_resize_img_s", "kernels": "kernel_us_per_image"}[kind]][b] = val
    print(json.dumps(out))
    sys.exit(0)

import numpy as np
import torch
import __graft_entry__
__graft_entry__.build(only_library=True)
import bench
import eval_disp
import test_disp
import supervised_dispnet_amd.models as models
import supervised_dispnet_amd.utils as U
from supervised_dispnet_amd import _lib, evaluation as EV, kitti_eval as KE

dev = torch.device("cuda:0")
kind, _, B = a.step.partition(":")
B = int(B or 1)
H, W, h, w = 375, 1242, 128, 416
r = np.random.RandomState(0)
args = eval_disp.parse_args(["--network", "disp_vgg_BN", "--pretrained-dispnet", "none", "--unsupervised"] +
                           (["--eval-batch", str(B), "--device-resize"] if kind == "resize" else []))
torch.manual_seed(0)
net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
bench._quiet_init(net)
net.to(dev).eval()


def fabricate(n):
    out = []
    for _ in range(n):
        gt = np.where(r.rand(H, W) < 0.05, r.uniform(1, 79, (H, W)), 0.0)
        u8 = r.randint(0, 256, (H, W, 3)).astype(np.uint8)          # as KittiTestFramework hands a frame over
        out.append({"tgt": u8.astype(np.float32), "tgt_u8": u8, "gt_depth": gt, "mask": KE.generate_mask(gt, 1e-3, 80)})
    return out


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


with torch.no_grad():
    if kind == "host":
        samples = fabricate(a.samples)
        print(json.dumps(rate(lambda: [test_disp.evaluate_sample(args, net, s, dev, 1e-3, 80, KE, U) for s in samples], len(samples))))
    elif kind in ("device", "resize"):
        samples = fabricate(a.samples)
        ev = EV.DeviceEvaluator(args, net, dev, 1e-3, 80)
        print(json.dumps(rate(lambda: [ev.evaluate(samples[j:j + B]) for j in range(0, len(samples), B)], len(samples))))
    else:
        samples = fabricate(B)
        st = torch.cuda.current_stream().cuda_stream
        hw, off, npix, total = EV.ragged_layout([(H, W)] * B)
        depth = torch.rand((B, h, w), device=dev) * 60 + 1
        coef = torch.empty((B, h, w), dtype=torch.float64, device=dev)
        zoomed = torch.empty(total, device=dev)
        d_hw, d_off, d_npix = (torch.from_numpy(x).to(dev) for x in (hw, off, npix))
        d_gt = torch.from_numpy(EV.pack_ragged([s["gt_depth"] for s in samples], np.float32, off, total)).to(dev)
        d_mask = torch.from_numpy(EV.pack_ragged([s["mask"] for s in samples], np.uint8, off, total)).to(dev)
        res = torch.empty((B, 8), device=dev)
        steps = {
            "prefilter": lambda: _lib.call("dn_zoom3_prefilter", depth.data_ptr(), B, h, w, coef.data_ptr(), st),
            "zoom": lambda: _lib.call("dn_zoom3_clip", coef.data_ptr(), B, h, w, d_hw.data_ptr(), d_off.data_ptr(), H, W, 1e-3, 80.0,
                                      zoomed.data_ptr(), st),
            "errors": lambda: _lib.call("dn_eval_errors", d_gt.data_ptr(), zoomed.data_ptr(), d_mask.data_ptr(), d_off.data_ptr(),
                                        d_npix.data_ptr(), B, EV.SCALE_MEDIAN, 1.0, res.data_ptr(), st),
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
