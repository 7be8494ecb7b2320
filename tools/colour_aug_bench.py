#!/usr/bin/env python3
"""Kernel time per batch of the shard path's image kernels without the colour jitter, with it and with keep_plain, and the rate of the
host chain the GPU path replaces, in ONE process.

    python tools/colour_aug_bench.py [--batch 32] [--height 128] [--width 416] [--frames 2] [--repeats 5] [--window-s 0.5] [--out FILE.json]

GPU modes, on resident uint8 frames [1 + frames][batch][H][W][3] (the depth's dn_flip_w is the same launch in every mode and left out),
each recorded once on the library's launch tape and timed as device time between two events around a window of replays, every window
warmed first, `repeats` windows per mode, ALTERNATING between the modes (the scheme of tools/reproj_bench.py); printed per mode: every
window, the median and the spread (max - min) between repeats:
  * plain:            dn_u8_normalize_flip, one launch per image of the sample (ShardLoader without color_aug);
  * jitter:           dn_colour_jitter_sums + dn_colour_jitter_normalize_flip, the samples jittered as data.draw_colour_jitter draws them
                      (about half);
  * jitter+plain:     the same with the plain frames written too (keep_plain);
  * jitter, all:      every sample jittered (the cost of the chain itself).
Host: data.colour_jitter_u8 (Pillow) on the same frames, every frame jittered, in a pool of processes over the box's cores (at most 16),
forked BEFORE the GPU is touched; frames per second over all workers and per worker.
The bytes per pixel are counted from the shapes (3 read; 12 or 24 written; the sums read 3 more), not measured.  One JSON line at the end."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_FRAMES = _BARRIER = None


def _host_init(barrier):
    global _BARRIER
    _BARRIER = barrier


def _host_worker(job):
    """jitter `count` frames starting at `first`; returns the seconds it took"""
    from supervised_dispnet_amd import data as D
    first, count, seed = job
    rng = np.random.RandomState(seed)
    params = [D.draw_colour_jitter(rng, prob=-1.0) for _ in range(count)]                   # prob < 0: every draw jitters
    D.colour_jitter_u8(_FRAMES[first % len(_FRAMES)], params[0])                            # imports, first call
    _BARRIER.wait()                                                                         # every worker times the same stretch
    t0 = time.perf_counter()
    for i, p in enumerate(params):
        D.colour_jitter_u8(_FRAMES[(first + i) % len(_FRAMES)], p)
    return time.perf_counter() - t0


def host_rate(frames, per_worker):
    global _FRAMES
    _FRAMES = frames
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    ctx = multiprocessing.get_context("fork")
    with ctx.Pool(workers, initializer=_host_init, initargs=(ctx.Barrier(workers),)) as pool:
        secs = pool.map(_host_worker, [(k * per_worker, per_worker, k) for k in range(workers)], chunksize=1)
    return {"workers": workers, "frames_per_worker": per_worker, "frames_per_s_per_worker": round(per_worker / statistics.median(secs), 1),
            "frames_per_s_all_workers": round(workers * per_worker / max(secs), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--frames", type=int, default=2, help="reference frames per sample")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--host-frames", type=int, default=48, help="frames each host worker jitters")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    b, h, w, n = args.batch, args.height, args.width, 1 + args.frames
    u8 = np.random.RandomState(0).randint(0, 256, (n, b, h, w, 3)).astype(np.uint8)
    host = host_rate(u8.reshape(n * b, h, w, 3), args.host_frames)                          # before the GPU is opened: the workers are forks
    print("host chain", host, flush=True)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("colour_aug_bench: needs the GPU (no fallback: a CPU timing says nothing about it)")
    import bench
    from supervised_dispnet_amd import _lib, data as D, shards as S
    dev = torch.device("cuda:0")
    lib = _lib.load()
    mean, std = D.normalization()
    mh, sh = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    md, sd = torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    d_u8 = torch.from_numpy(u8).to(dev)
    d_fl = torch.from_numpy((np.arange(b) % 2).astype(np.uint8)).to(dev)
    rng = np.random.RandomState(0)
    drawn = [D.draw_colour_jitter(rng) for _ in range(b)]
    every = [D.draw_colour_jitter(rng, prob=-1.0) for _ in range(b)]

    def table(params):
        tb = np.zeros((b, S.COLOUR_PARAMS), dtype=np.int32)
        for row, p in zip(tb, params):
            S.colour_params_row(p, row)
        return torch.from_numpy(tb).to(dev)

    t_drawn, t_every = table(drawn), table(every)
    sums = torch.empty((n * b, 64), dtype=torch.int64, device=dev)
    out = torch.empty((n, b, 3, h, w), dtype=torch.float32, device=dev)
    plain = torch.empty_like(out)
    side = torch.cuda.Stream(device=dev)
    st = side.cuda_stream

    def run_plain():
        for i in range(n):
            _lib.call("dn_u8_normalize_flip", d_u8[i].data_ptr(), d_fl.data_ptr(), b, h, w, 3, md.data_ptr(), sd.data_ptr(), mh, sh,
                      out[i].data_ptr(), 3 * h * w, h * w, st)

    def run_jitter(tb, keep):
        _lib.call("dn_colour_jitter_sums", d_u8.data_ptr(), tb.data_ptr(), n, b, h, w, sums.data_ptr(), st)
        _lib.call("dn_colour_jitter_normalize_flip", d_u8.data_ptr(), d_fl.data_ptr(), tb.data_ptr(), sums.data_ptr(), n, b, h, w, mh, sh,
                  out.data_ptr(), plain.data_ptr() if keep else None, st)

    modes = {"plain (%d x dn_u8_normalize_flip)" % n: run_plain,
             "jitter (%d of %d samples)" % (sum(p is not None for p in drawn), b): lambda: run_jitter(t_drawn, False),
             "jitter + plain": lambda: run_jitter(t_drawn, True),
             "jitter, every sample": lambda: run_jitter(t_every, False)}
    torch.cuda.synchronize()
    tapes, launches = {}, {}
    for name, fn in modes.items():
        fn()
        side.synchronize()
        tape = lib.dn_tape_begin()
        if not tape:
            raise SystemExit("dn_tape_begin: " + _lib.last_error())
        fn()
        _lib.check(lib.dn_tape_end(tape), "dn_tape_end")
        tapes[name], launches[name] = tape, int(lib.dn_tape_launches(tape))
    side.synchronize()

    def window(tape, seconds):
        for _ in range(3):
            _lib.check(lib.dn_tape_replay(tape, -1), "dn_tape_replay")
        side.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        count, total = 0, 0.0
        while total < seconds * 1e3:
            e0.record(side)
            for _ in range(20):
                _lib.check(lib.dn_tape_replay(tape, -1), "dn_tape_replay")
            e1.record(side)
            e1.synchronize()
            total += e0.elapsed_time(e1)
            count += 20
        return total / count

    times = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name in modes:
            times[name].append(window(tapes[name], args.window_s))
    for tape in tapes.values():
        lib.dn_tape_free(tape)
    px = n * b * h * w
    bpp = {"plain": 15, "jitter": 18, "jitter + plain": 30}
    result = {"tool": "colour_aug_bench", "size": [b, h, w], "images_per_sample": n, "window_s": args.window_s, "repeats": args.repeats,
              "host": bench.host_description(), "device": torch.cuda.get_device_name(0), "bytes_per_pixel": bpp, "host_chain": host, "modes": {}}
    for name in modes:
        ms = times[name]
        med = statistics.median(ms)
        nbytes = px * (15 if name.startswith("plain") else (30 if "+ plain" in name else 18))
        entry = {"ms": [round(v, 4) for v in ms], "median_ms": round(med, 4), "spread_ms": round(max(ms) - min(ms), 4), "launches": launches[name],
                 "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
        result["modes"][name] = entry
        print("%-34s median %.4f ms  spread %.4f ms  (%s)  launches %d  %.2f TB/s" % (name, entry["median_ms"], entry["spread_ms"],
                                                                                      " ".join("%.4f" % v for v in ms), launches[name], entry["TB_per_s"]), flush=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
