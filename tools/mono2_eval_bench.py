#!/usr/bin/env python3
"""What does eval_disp.py --protocol monodepth2 cost, and what does --eval-batch buy under it?  Fabricates in-memory KITTI-shaped samples
(375 x 1242 frame, ~5 %-dense ground truth, Garg-crop mask) and a freshly initialised monodepth2 ResnetEncoder(18) + DepthDecoder at
128 x 416, and reports

  chain, with and without --post-process: images per second of the per-image host chain (evaluation.mono2_evaluate_sample: forward at
      batch 1 or 2, copy back, numpy post-process / resize / metrics) and of the DeviceEvaluator at batch 1 / 8 / 32.  The candidates
      ALTERNATE: every round runs one window of each, a window is one pass over all samples and ends in a device synchronise;
  kernels: device time per image (HIP events around 50 launches, in microseconds) of dn_mono2_post_process, dn_bilinear_recip_ragged and
      dn_eval_errors_clamp on resident data at batch 1 / 8 / 32, 128 x 416 -> 375 x 1242, alternating in the same way.

Every window is printed, then its candidate's median and spread (min .. max); the last line is one JSON object with all windows.  Both
chains include the resize of the frame on the host; neither includes reading files.  Each of the three measurements is a child process
of its own under a time limit; the first one that fails ends the run.

usage: python tools/mono2_eval_bench.py [--samples 64] [--rounds 5] [--timeout 420]"""
import argparse, json, pathlib, statistics, subprocess, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5, help="windows per candidate")
ap.add_argument("--timeout", type=int, default=420, help="seconds per measurement")
ap.add_argument("--step", default=None, help="(internal) chain:0 | chain:1 | kernels")
a = ap.parse_args()
BATCHES = (1, 8, 32)


def summary(vals):
    return "median %.4g  min %.4g  max %.4g  spread %.1f %%" % (statistics.median(vals), min(vals), max(vals),
                                                               100 * (max(vals) - min(vals)) / statistics.median(vals))


if a.step is None:
    out = {"samples": a.samples, "rounds": a.rounds, "network": "monodepth2 ResnetEncoder(18) + DepthDecoder 128x416", "gt": [375, 1242]}
    for step, key in (("chain:0", "img_s"), ("chain:1", "img_s_post_process"), ("kernels", "kernel_us_per_image")):
        cmd = [sys.executable, __file__, "--step", step, "--samples", str(a.samples), "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, text=True)     # a fresh process per step; raises on a time-out
        sys.stdout.write("".join(line + "\n" for line in p.stdout.splitlines()[:-1]))
        if p.returncode != 0:
            raise SystemExit("%s failed with status %d" % (step, p.returncode))
        out[key] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    sys.exit(0)

import numpy as np
import torch
import __graft_entry__
__graft_entry__.build(only_library=True)
import eval_disp
import supervised_dispnet_amd.models as models
import supervised_dispnet_amd.networks as networks
from supervised_dispnet_amd import _lib, evaluation as EV, kitti_eval as KE

if not torch.cuda.is_available():
    raise SystemExit("mono2_eval_bench.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
kind, _, pp = a.step.partition(":")
pp = pp == "1"
H, W, h, w = 375, 1242, 128, 416
r = np.random.RandomState(0)


def fabricate(n):
    out = []
    for _ in range(n):
        gt = np.where(r.rand(H, W) < 0.05, r.uniform(1, 79, (H, W)), 0.0)
        u8 = r.randint(0, 256, (H, W, 3)).astype(np.uint8)          # as KittiTestFramework hands a frame over
        out.append({"tgt": u8.astype(np.float32), "tgt_u8": u8, "gt_depth": gt, "mask": KE.generate_mask(gt, 1e-3, 80)})
    return out


def report(title, unit, windows):
    for name, vals in windows.items():
        for i, v in enumerate(vals):
            print("%s  %-28s window %d: %10.4g %s" % (title, name, i, v, unit))
    for name, vals in windows.items():
        print("%s  %-28s %s" % (title, name, summary(vals)))
    print(json.dumps(windows))


with torch.no_grad():
    if kind == "chain":
        args = eval_disp.parse_args(["--network", "disp_res_18", "--pretrained-dispnet", "none", "--mono", "--protocol", "monodepth2"] +
                                   (["--post-process"] if pp else []))
        torch.manual_seed(0)
        enc = networks.ResnetEncoder(18, False)
        net = models.monodepth2(encoder=enc, decoder=networks.DepthDecoder(enc.num_ch_enc)).to(dev).eval()
        samples = fabricate(a.samples)
        ev = EV.DeviceEvaluator(args, net, dev, 1e-3, 80)
        cands = {"host chain": lambda: [EV.mono2_evaluate_sample(args, net, s, dev, 1e-3, 80, pp) for s in samples]}
        for B in BATCHES:
            cands["device chain, batch %d" % B] = lambda B=B: [ev.evaluate(samples[j:j + B]) for j in range(0, len(samples), B)]
        for fn in cands.values():          # warm-up pass of every candidate
            fn()
        windows = {k: [] for k in cands}
        for _ in range(a.rounds):
            for name, fn in cands.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                windows[name].append(len(samples) / (time.perf_counter() - t0))
        report("post-process %s" % ("on " if pp else "off"), "images/s", windows)
    else:
        st = torch.cuda.current_stream().cuda_stream
        cands = {}
        keep = []
        for B in BATCHES:
            samples = fabricate(B)
            hw, off, npix, total = EV.ragged_layout([(H, W)] * B)
            disp2 = torch.rand((2 * B, h, w), device=dev) * 9.99 + 0.01
            disp = torch.empty((B, h, w), device=dev)
            depth = torch.empty(total, device=dev)
            d_hw, d_off, d_npix = (torch.from_numpy(x).to(dev) for x in (hw, off, npix))
            d_gt = torch.from_numpy(EV.pack_ragged([s["gt_depth"] for s in samples], np.float32, off, total)).to(dev)
            d_mask = torch.from_numpy(EV.pack_ragged([s["mask"] for s in samples], np.uint8, off, total)).to(dev)
            res = torch.empty((B, 8), device=dev)
            keep.append((disp2, disp, depth, d_hw, d_off, d_npix, d_gt, d_mask, res))
            cands["post_process, batch %d" % B] = (B, lambda B=B, t=keep[-1]: _lib.call("dn_mono2_post_process", t[0].data_ptr(), B, h, w, t[1].data_ptr(), st))
            cands["resize_recip, batch %d" % B] = (B, lambda B=B, t=keep[-1]: _lib.call("dn_bilinear_recip_ragged", t[1].data_ptr(), B, h, w, t[3].data_ptr(),
                                                                                       t[4].data_ptr(), H, W, t[2].data_ptr(), st))
            cands["errors_clamp, batch %d" % B] = (B, lambda B=B, t=keep[-1]: _lib.call("dn_eval_errors_clamp", t[6].data_ptr(), t[2].data_ptr(), t[7].data_ptr(),
                                                                                       t[4].data_ptr(), t[5].data_ptr(), B, EV.SCALE_MEDIAN, 1.0, 1e-3, 80.0,
                                                                                       t[8].data_ptr(), st))
        for _, fn in cands.values():       # warm-up, in dependency order: every later input is a real depth map
            fn()
        torch.cuda.synchronize()

        def timed(fn, B, reps=50):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / reps / B

        windows = {k: [] for k in cands}
        for _ in range(a.rounds):
            for name, (B, fn) in cands.items():
                windows[name].append(timed(fn, B))
        report("kernels", "us/image", windows)
