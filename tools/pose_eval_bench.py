#!/usr/bin/env python3
"""What does eval_pose.py's device chain buy?  Writes a synthetic odometry sequence (200 frames of 376 x 1241 as PNG, a smooth closed-form
trajectory) into a temporary directory and measures, on freshly initialised networks at 128 x 416,

  snippets_s       snippets (poseexp, L = 5) / pairs (resnet18) per second of one whole evaluate() of the sequence -- reading the files,
                   resizing, forward, metric -- for --host-chain and for the device chain at batch 1 / 8 / 32.  The candidates alternate
                   inside each of the --windows windows (after one warm-up round); reported: the median and the spread (min .. max).
  kernel_us        HIP-event time per launch of dn_snippet_gather and of the metric kernel on resident data, per batch size
                   (dn_pose_eval_mono2: one launch over the whole sequence).

One JSON line; --out FILE also writes a small table (profiles/pose_eval_bench.txt).  No speed-up is promised: the numbers are what
they are.

usage: python tools/pose_eval_bench.py [--frames 200] [--windows 5] [--readers 4] [--out profiles/pose_eval_bench.txt]"""
import argparse, json, os, pathlib, statistics, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--readers", type=int, default=4)
ap.add_argument("--models", nargs="*", default=["poseexp", "resnet18"])
ap.add_argument("--out", default=None)
a = ap.parse_args()
BATCHES = (1, 8, 32)
RAW, NET = (376, 1241), (128, 416)

import numpy as np
import torch
import __graft_entry__
__graft_entry__.build(only_library=True)
import supervised_dispnet_amd.models as models
import supervised_dispnet_amd.networks as networks
from supervised_dispnet_amd import _lib, pose_eval as PE

dev = torch.device("cuda:0")


def write_sequence(root, n):
    from PIL import Image
    folder = os.path.join(root, "sequences", "00", "image_2")
    os.makedirs(folder)
    os.makedirs(os.path.join(root, "poses"))
    y, x = np.meshgrid(np.arange(RAW[0]), np.arange(RAW[1]), indexing="ij")
    poses = np.zeros((n, 3, 4))
    for k in range(n):
        img = np.stack([(127 + 100 * np.sin(0.02 * x + 0.1 * k + c) * np.cos(0.03 * y + 0.05 * c * k) + 20 * ((x // 8 + y // 8 + k) % 2)) for c in range(3)], 2)
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(os.path.join(folder, "%06d.png" % k), compress_level=1)
        ang = 0.01 * k
        poses[k, :, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        poses[k, :, 3] = [np.sin(ang) * 50, 0.01 * k, 0.8 * k]
    np.savetxt(os.path.join(root, "poses", "00.txt"), poses.reshape(n, 12), fmt="%.12e")
    return PE.read_sequence(root, "00")


def make_net(name):
    torch.manual_seed(0)
    if name == "poseexp":
        net = models.PoseExpNet(nb_ref_imgs=4, output_exp=False)
        net.init_weights()
        return net.to(dev).eval(), "sfmlearner", 5
    return networks.PoseResnet(18).to(dev).eval(), "monodepth2", 2


def kernel_times(protocol, L, count, reps=20):
    st = torch.cuda.current_stream().cuda_stream
    import ctypes
    mean, std = PE.normalization(protocol)
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    out = {}

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps

    for B in BATCHES:
        R = B + L - 1
        ring = torch.randint(0, 256, (R, NET[0], NET[1], 3), dtype=torch.uint8, device=dev)
        idx = (torch.arange(B, dtype=torch.int32, device=dev)[:, None] + torch.arange(L, dtype=torch.int32, device=dev)[None, :]).contiguous()
        dense = torch.empty((B, 3 * L, NET[0], NET[1]), dtype=torch.float32, device=dev)
        val = {"gather": timed(lambda: _lib.call("dn_snippet_gather", ring.data_ptr(), R, idx.data_ptr(), B, L, NET[0], NET[1], m, s, dense.data_ptr(), st))}
        if protocol == "sfmlearner":
            pose = torch.randn((B, L - 1, 6), device=dev) * 0.05
            gt = torch.randn((B, L, 3, 4), dtype=torch.float64, device=dev)
            res = torch.empty((B, 2), dtype=torch.float64, device=dev)
            val["metric"] = timed(lambda: _lib.call("dn_pose_eval_sfm", pose.data_ptr(), 0, gt.data_ptr(), B, L, res.data_ptr(), st))
        out[str(B)] = val
    if protocol == "monodepth2":
        pose = torch.randn((count, 6), device=dev) * 0.05
        Q = torch.eye(4, dtype=torch.float64, device=dev).repeat(count, 1, 1).contiguous()
        Q[:, 2, 3] = 0.8
        res = torch.empty((count,), dtype=torch.float64, device=dev)
        out["sequence"] = {"metric": timed(lambda: _lib.call("dn_pose_eval_mono2", pose.data_ptr(), Q.data_ptr(), count, PE.TRACK_LENGTH, res.data_ptr(), st))}
    return out


result = {"frames": a.frames, "raw": list(RAW), "network_size": list(NET), "windows": a.windows, "readers": a.readers, "models": {}}
with tempfile.TemporaryDirectory() as tmp:
    files, poses = write_sequence(tmp, a.frames)
    for name in a.models:
        net, protocol, L = make_net(name)
        cands = {"host": PE.HostPoseEvaluator(net, protocol, dev, NET)}
        for B in BATCHES:
            cands["device:%d" % B] = PE.DevicePoseEvaluator(net, protocol, dev, NET, B, readers=a.readers, keep_raw=False)
        rates = {k: [] for k in cands}
        count = None
        for w in range(a.windows + 1):                     # round 0 warms every candidate up
            for k, ev in cands.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                errors, _ = ev.evaluate(files, poses, L)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                count = len(errors)
                if w:
                    rates[k].append(count / dt)
                print("%s window %d %s: %.1f /s" % (name, w, k, count / dt), file=sys.stderr, flush=True)
        result["models"][name] = {"protocol": protocol, "L": L, "count": count,
                                  "snippets_s": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rates.items()},
                                  "kernel_us": kernel_times(protocol, L, count)}
print(json.dumps(result))
if a.out:
    lines = ["pose_eval_bench: %d frames of %d x %d -> %d x %d, %d windows, candidates alternating, %d reader threads" % (
        a.frames, RAW[0], RAW[1], NET[0], NET[1], a.windows, a.readers), ""]
    for name, r in result["models"].items():
        lines.append("%s (%s, L = %d, %d %s per sequence)" % (name, r["protocol"], r["L"], r["count"], "snippets" if r["L"] > 2 else "pairs"))
        lines.append("  %-12s %12s %12s %12s" % ("chain", "median /s", "min /s", "max /s"))
        for k, v in r["snippets_s"].items():
            lines.append("  %-12s %12.1f %12.1f %12.1f" % (k, v["median"], v["min"], v["max"]))
        for b, v in r["kernel_us"].items():
            lines.append("  kernels, batch %-8s %s" % (b, "  ".join("%s %.1f us" % kv for kv in v.items())))
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
