#!/usr/bin/env python3
"""Kernel time of loss_functions.min_reprojection_loss, forward + backward, in ONE process.

    python tools/reproj_bench.py [--batch 32] [--height 128] [--width 416] [--frames 2] [--repeats 5] [--window-s 0.5] [--out FILE.json]

Timed per mode (automask on / off): the loss forward and its backward (graph.backward: gradients to the disparity and to every T) on
fixed closed-form tensors, as device time between two events around `window` iterations, every window warmed first; `repeats`
windows per mode, ALTERNATING between the modes.  Printed per mode: the time of every window, the median and the spread (max - min)
between repeats -- the yardstick any difference has to beat -- and the launches per forward + backward a launch tape records (the
timed thing is the replay of that tape).  For
orientation the same measurement of photometric_reconstruction_loss at its scale 0 on the same images (SfMLearner's term: one warp +
L1 per frame, no SSIM, no minimum; 6-vector poses).  No threshold applies: there is no earlier path to beat.  The bytes per pixel
are counted from the shapes (each operand read once, each result written once), not measured.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bytes_per_pixel(frames, automask):
    """fp32 bytes per target pixel, algorithmic: forward = per frame the warped term (tgt 12 + ref 12 + disp 4 read, term 4 written) and
    the identity term (24 read, 4 written), then the select (terms read, m 4 + selection 1 written); backward = per frame the coefficient
    pass (tgt, ref, disp, selection read; 36 written) and the gather pass (the same reads + 36 of coefficients; ddisp 4 written, re-read
    for the frames after the first)."""
    nch = (2 if automask else 1) * frames
    fwd = frames * 32 + (frames * 28 if automask else 0) + 4 * nch + 5
    bwd = frames * ((29 + 36) + (29 + 36 + 4)) + 4 * (frames - 1)
    return {"forward": fwd, "backward": bwd}


def smooth_images(b, h, w, dev, frames):
    y = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    ph = torch.arange(b * 3, dtype=torch.float64).view(b, 3, 1, 1) * 0.37

    def img(dx, dy):
        return (0.5 + 0.2 * torch.sin(0.23 * (x - dx) + 0.11 * (y - dy) + ph) + 0.15 * torch.sin(-0.09 * (x - dx) + 0.31 * (y - dy) + 2 * ph)).float().to(dev)

    tgt = img(0, 0)
    refs = [img(1.5 * (-1) ** f, 0.5 * f) for f in range(frames)]
    disp = (0.02 + 0.03 * (0.5 + 0.5 * torch.sin(0.05 * x + 0.045 * y + ph[:, :1]))).float().to(dev)
    return tgt, refs, disp


def window(fn, seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 0, 0.0
    while total < seconds * 1e3:
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
        n += 10
    return total / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reproj_bench: needs the GPU (no fallback: a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    import bench
    import supervised_dispnet_amd.loss_functions as LF
    from supervised_dispnet_amd.graph import TapedStep, backward
    b, h, w, nf = args.batch, args.height, args.width, args.frames
    tgt, refs, disp0 = smooth_images(b, h, w, dev, nf)
    fx, fy, cx, cy = 241.67 * w / 416, 246.28 * h / 128, 204.17 * w / 416, 59.0 * h / 128
    K = torch.tensor([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32).repeat(b, 1, 1)
    Kinv = torch.inverse(K.double()).float().contiguous().to(dev)
    K = K.to(dev)
    T = []
    for f in range(nf):
        t = torch.eye(4).repeat(b, 1, 1)
        t[:, 0, 3], t[:, 1, 3] = 0.1 * (-1) ** f, 0.02 * f
        T.append(t.to(dev).requires_grad_())
    disp = disp0.clone().requires_grad_()
    pose6 = torch.zeros(b, nf, 6)
    for f in range(nf):
        pose6[:, f, 0], pose6[:, f, 1] = 0.1 * (-1) ** f, 0.02 * f
    pose6 = pose6.to(dev).requires_grad_()
    depth = (1 / (0.01 + 9.99 * disp0)).requires_grad_()
    K3, K3inv = K[:, :3, :3].contiguous(), Kinv[:, :3, :3].contiguous()

    def reproj(automask):
        def fn():
            disp.grad = None
            for t in T:
                t.grad = None
            backward(LF.min_reprojection_loss(tgt, refs, disp, K, Kinv, T, automask=automask))
        return fn

    def photo():
        depth.grad = None
        pose6.grad = None
        backward(LF.photometric_reconstruction_loss(tgt, refs, K3, K3inv, [depth], [None], pose6, "euler", "border"))

    modes = {"min_reprojection_loss, automask": reproj(True), "min_reprojection_loss, no automask": reproj(False),
             "photometric_reconstruction_loss, scale 0": photo}
    # the fused loss is timed as a launch-tape replay (the host then spends ~2 us per launch and the events bracket kernel time); the
    # photometric loss allocates its accumulators with framework fills, which a tape would miss: it is timed eagerly
    launches, timed, tapes = {}, {}, []
    for name, fn in modes.items():
        if name.startswith("min_reprojection"):
            ts = TapedStep(fn, warmup=1).capture()
            launches[name], timed[name] = int(ts.launches), ts
            tapes.append(ts)
        else:
            launches[name], timed[name] = 2 * nf + 2 * nf + nf + 1, fn        # proj + warp, finalize | warp backward + pose backward, per frame
    times = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name in modes:
            times[name].append(window(timed[name], args.window_s))
    for ts in tapes:
        ts.close()
    result = {"tool": "reproj_bench", "size": [b, h, w], "frames": nf, "window_s": args.window_s, "repeats": args.repeats,
              "host": bench.host_description(), "device": torch.cuda.get_device_name(0), "tile": [8, 32], "lds_bytes_per_block": 6 * 340 * 4 + 48,
              "modes": {}}
    for name in modes:
        ms = times[name]
        entry = {"ms": [round(v, 4) for v in ms], "median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
                 "launches_fwd_bwd": launches[name]}
        if name.startswith("min_reprojection"):
            bp = bytes_per_pixel(nf, "no automask" not in name)
            entry["bytes_per_pixel"] = bp
            entry["algorithmic_GBps"] = round((bp["forward"] + bp["backward"]) * b * h * w / (entry["median_ms"] * 1e-3) / 1e9, 1)
        result["modes"][name] = entry
        print("%-42s median %.4f ms  spread %.4f ms  (%s)  launches %d" % (name, entry["median_ms"], entry["spread_ms"],
                                                                          " ".join("%.4f" % v for v in ms), launches[name]), flush=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
