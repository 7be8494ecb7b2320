#!/usr/bin/env python3
"""Train-mode step against the --freeze-bn step of Disp_vgg_BN 128x416, through the launch tape, in ONE process.

    python tools/frozen_bn_bench.py [--batches 32 4] [--repeats 5] [--window-s 1.0] [--out FILE.json]

Per batch size two networks with the same weights are built, one with every BatchNorm in eval mode (train.py --freeze-bn); each step
(forward + 1/disp + L1 + backward + fused Adam) is recorded on a launch tape (graph.TapedStep) and checked against the eager step bit for
bit.  Then the two tapes are timed ALTERNATELY, `repeats` times each: every window is warmed, replays until at least `window-s`
seconds have passed and ends in a device synchronise (host clock around it).  Printed per mode: the step time of every window, the
median and the spread (max - min) between repeats of the SAME step -- the yardstick a difference between the modes has to beat --, the
launches and fences per step the tape recorded, and the bytes each BatchNorm-backward form moves per element (counted from the shapes,
not measured).  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# fp32 bytes per element of the full-resolution pre-BatchNorm map each BatchNorm backward moves (reads + writes of full-size tensors;
# per-channel vectors and partial rows are noise).  Pool forms: the pooled gradient is a quarter of a map, the codes a sixteenth.
BYTES_PER_ELEMENT = {
    "train, ReLU pending, sums fused into the input-gradient epilogue": {"passes": 1, "bytes": 12, "what": "apply: read da, y; write dy (+ y re-read by the epilogue of the layer above: 4)"},
    "train, ReLU pending, own sums pass": {"passes": 2, "bytes": 20, "what": "sums: read da, y (8); apply: read da, y, write dy (12)"},
    "train, through the 2x2 max-pool": {"passes": 2, "bytes": 5.25 + 9.25, "what": "sums: read dpooled (1), idx (.25), y (4); apply: the same reads + write dy (4)"},
    "train, residual tail with downsample": {"passes": 3, "bytes": 24 + 12 + 12, "what": "tail: read gout, out, y, r, write dz, dr (24); one apply per branch (12 each)"},
    "frozen, ReLU pending or dz given": {"passes": 1, "bytes": 12, "what": "read g, y; write dy (sums in the same pass)"},
    "frozen, through the 2x2 max-pool": {"passes": 1, "bytes": 9.25, "what": "read dpooled (1), idx (.25), y (4); write dy (4)"},
    "frozen, residual tail with downsample": {"passes": 1, "bytes": 24, "what": "read gout, out, y, r; write dy, dr"},
    "frozen, residual tail with identity": {"passes": 1, "bytes": 20, "what": "read gout, out, y; write dy; write (or read and write: 24) the identity's gradient"},
}


def build(batch, h, w, dev, frozen, sd0):
    import bench
    import supervised_dispnet_amd.loss_functions as LF
    import supervised_dispnet_amd.models as models
    from supervised_dispnet_amd.functional import reciprocal
    from supervised_dispnet_amd.graph import TapedStep, backward
    from supervised_dispnet_amd.optim import FusedAdam
    torch.manual_seed(0)
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    bench._quiet_init(net)
    if sd0 is not None:
        net.load_state_dict(sd0)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    net.to(dev).train()
    if frozen:
        for m in net.modules():
            if m.__class__.__name__.find("BatchNorm") != -1:
                m.eval()
    opt = FusedAdam(net._hot_parameters(), lr=1e-4, production_order=net._grad_production_order())
    batches = [bench.synthetic_batch(batch, h, w, dev, seed) for seed in range(2)]
    img, gt = batches[0][0].clone(), batches[0][1].clone()

    def step():
        depth = [reciprocal(d) for d in net(img)]
        loss = LF.l1_loss(gt, depth, "kitti")
        opt.zero_grad()
        backward(loss)
        opt.step()
        return loss

    ts = TapedStep(step, optimizer=opt, warmup=2, static_inputs=(img, gt))
    ts.capture()
    img.copy_(batches[1][0])
    gt.copy_(batches[1][1])
    same, worst = ts.verify(opt.tape_state() + [b for b in net.buffers() if b.is_cuda])
    return ts, {"launches": int(ts.launches), "fences": int(ts.fences), "segments": int(ts.segments), "replay_is_eager_bitwise": bool(same),
                "max_abs_diff": float(worst)}, sd, (net, opt, img, gt)


def window(ts, seconds, warm=5):
    for _ in range(warm):
        ts()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(10):
            ts()
        n += 10
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 4])
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_bn_bench: needs the GPU (no fallback: a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    import bench
    result = {"tool": "frozen_bn_bench", "network": "Disp_vgg_BN", "size": [args.height, args.width], "window_s": args.window_s,
              "repeats": args.repeats, "host": bench.host_description(), "device": torch.cuda.get_device_name(0), "batches": {},
              "bn_backward_bytes_per_element": BYTES_PER_ELEMENT}
    for b in args.batches:
        ts_t, info_t, sd0, keep_t = build(b, args.height, args.width, dev, False, None)
        ts_f, info_f, _, keep_f = build(b, args.height, args.width, dev, True, sd0)
        times = {"train": [], "frozen": []}
        for _ in range(args.repeats):
            times["train"].append(window(ts_t, args.window_s))
            times["frozen"].append(window(ts_f, args.window_s))
        entry = {}
        for mode, info in (("train", info_t), ("frozen", info_f)):
            ms = [1e3 * t for t in times[mode]]
            entry[mode] = dict(info, step_ms=[round(v, 4) for v in ms], median_ms=round(statistics.median(ms), 4),
                               spread_ms=round(max(ms) - min(ms), 4), images_per_s=round(b / (statistics.median(ms) * 1e-3), 1))
            print("b%-3d %-6s median %.4f ms  spread %.4f ms  (%s)  launches %d fences %d  replay==eager %s" % (
                b, mode, entry[mode]["median_ms"], entry[mode]["spread_ms"], " ".join("%.4f" % v for v in ms), info["launches"], info["fences"],
                info["replay_is_eager_bitwise"]), flush=True)
        d = entry["frozen"]["median_ms"] - entry["train"]["median_ms"]
        spread = max(entry["train"]["spread_ms"], entry["frozen"]["spread_ms"])
        entry["frozen_minus_train_ms"] = round(d, 4)
        entry["frozen_not_slower_within_spread"] = bool(d <= spread)
        print("b%-3d frozen - train = %+.4f ms (spread between repeats of one step: %.4f ms)" % (b, d, spread), flush=True)
        result["batches"][str(b)] = entry
        ts_t.close()
        ts_f.close()
        del keep_t, keep_f
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
