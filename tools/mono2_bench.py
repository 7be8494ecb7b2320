#!/usr/bin/env python3
"""Kernel time of loss_functions.monodepth2_loss, forward + backward, against the same objective composed from single-scale pieces, in
ONE process.

    python tools/mono2_bench.py [--batch 32] [--height 128] [--width 416] [--frames 2] [--scales 4] [--repeats 5] [--window-s 0.5] [--out FILE.json]

Modes, timed as device time between two events around a window of iterations, every window warmed first, `repeats` windows per mode,
ALTERNATING between the modes (the scheme of tools/reproj_bench.py); printed per mode: every window, the median and the spread
(max - min) between repeats -- the yardstick a difference has to beat:
  * fused:     monodepth2_loss (automask, S scales) as the replay of a launch tape;
  * composed:  per scale _UpsampleInt -> min_reprojection_loss, framework arithmetic for the mean normalisation and the weighted sum,
               layers.get_smooth_loss -- the pieces that existed before the fused objective.  Its framework kernels cannot go on a
               launch tape, so it runs eagerly; the colour pyramid (F.interpolate, mode="area") is computed once OUTSIDE the timed
               region, which favours this mode;
  * min_reprojection_loss alone (one scale, launch tape), for scale.
The bytes per pixel are counted from the shapes (each operand read once, each result written once), not measured.  One JSON line at
the end."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reproj_bench import smooth_images, window  # noqa: E402


def bytes_per_pixel(frames, scales):
    """fp32 bytes per full-resolution pixel of the fused objective with automask; q = sum_s 4^-s is the size of the coarse maps.
    forward: per frame the identity term (24 read, 4 written) and the warped terms (per scale tgt 12 + ref 12 read, term 4 written; the
    coarse disparities 4 q), the select (F + F S terms read, S selection bytes written), the means (4 q) and the smoothness
    (tgt 12 per scale + 4 q read, its gradient 4 q written).  backward: per frame and scale the coefficient pass (tgt, ref, selection
    read; 36 written) and the gather pass (the same + 36 of coefficients; ddisp 4 written, re-read for the frames after the first),
    then the gather into the coarse maps (ddisp 4 per scale + the smoothness gradient 4 q read, 4 q written).
    workspace: the SSIM coefficients, 36 bytes per pixel per scale."""
    q = sum(0.25 ** s for s in range(scales))
    fwd = frames * 28 + frames * (scales * 28 + 4 * q) + 4 * (frames + frames * scales) + scales + 4 * q + (12 * scales + 8 * q)
    bwd = frames * scales * ((25 + 36) + (25 + 36 + 4)) + 4 * (frames - 1) * scales + (4 * scales + 8 * q)
    return {"forward": round(fwd, 1), "backward": round(bwd, 1), "workspace": 36 * scales}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--smoothness", type=float, default=1e-3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mono2_bench: needs the GPU (no fallback: a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    import torch.nn.functional as F
    import bench
    import supervised_dispnet_amd.layers as L
    import supervised_dispnet_amd.loss_functions as LF
    from supervised_dispnet_amd.graph import TapedStep, backward
    b, h, w, nf, S = args.batch, args.height, args.width, args.frames, args.scales
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
    disps = [(disp0 if s == 0 else F.interpolate(disp0, (h >> s, w >> s), mode="area")).contiguous().clone().requires_grad_() for s in range(S)]
    colours = [tgt if s == 0 else F.interpolate(tgt, (h >> s, w >> s), mode="area").contiguous() for s in range(S)]
    sm = args.smoothness

    def clear():
        for t in disps + T:
            t.grad = None

    def fused():
        clear()
        backward(LF.monodepth2_loss(tgt, refs, disps, K, Kinv, T, smoothness=sm))

    def composed():
        clear()
        total = 0
        for s, d in enumerate(disps):
            up = d if s == 0 else LF._UpsampleInt.apply(d, 2 ** s, 1)
            m = LF.min_reprojection_loss(tgt, refs, up, K, Kinv, T)
            norm = d / (d.mean((2, 3), keepdim=True) + 1e-7)
            total = total + m + (sm / 2 ** s) * L.get_smooth_loss(norm, colours[s])
        backward(total / S)

    def single():
        clear()
        backward(LF.min_reprojection_loss(tgt, refs, disps[0], K, Kinv, T))

    # the two forms agree (the fused one is not timed against something else)
    fused()
    g_f = [d.grad.clone() for d in disps]
    l_f = float(LF.monodepth2_loss(tgt, refs, disps, K, Kinv, T, smoothness=sm).detach())
    composed()
    l_c, total = 0.0, 0
    with torch.no_grad():
        for s, d in enumerate(disps):
            up = d if s == 0 else LF._UpsampleInt.apply(d, 2 ** s, 1)
            norm = d / (d.mean((2, 3), keepdim=True) + 1e-7)
            total = total + LF.min_reprojection_loss(tgt, refs, up, K, Kinv, T) + (sm / 2 ** s) * L.get_smooth_loss(norm, colours[s])
        l_c = float(total / S)
    agree = {"loss_fused": l_f, "loss_composed": l_c,
             "ddisp_rel_diff": [float((a - d.grad).abs().max() / d.grad.abs().max()) for a, d in zip(g_f, disps)]}
    print("agreement", agree, flush=True)

    modes = {"monodepth2_loss, fused (tape)": fused, "composed from single-scale pieces (eager)": composed,
             "min_reprojection_loss, one scale (tape)": single}
    launches, timed, tapes = {}, {}, []
    for name, fn in modes.items():
        if "tape" in name:
            ts = TapedStep(fn, warmup=1).capture()
            launches[name], timed[name] = int(ts.launches), ts
            tapes.append(ts)
        else:
            launches[name], timed[name] = None, fn
    times = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name in modes:
            times[name].append(window(timed[name], args.window_s))
    for ts in tapes:
        ts.close()
    result = {"tool": "mono2_bench", "size": [b, h, w], "frames": nf, "scales": S, "window_s": args.window_s, "repeats": args.repeats,
              "host": bench.host_description(), "device": torch.cuda.get_device_name(0), "agreement": agree,
              "bytes_per_pixel": bytes_per_pixel(nf, S), "workspace_MB": round(36 * S * b * h * w / 1e6, 1), "modes": {}}
    for name in modes:
        ms = times[name]
        entry = {"ms": [round(v, 4) for v in ms], "median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
                 "launches_fwd_bwd": launches[name]}
        result["modes"][name] = entry
        print("%-46s median %.4f ms  spread %.4f ms  (%s)  launches %s" % (name, entry["median_ms"], entry["spread_ms"],
                                                                          " ".join("%.4f" % v for v in ms), launches[name]), flush=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
