"""Kernel time of the fused optimizers over the Disp_vgg_BN arena: one dn_sgd_step next to one dn_adam_step, HIP events around
back-to-back launches on resident data, alternating between repeats.  All are HBM-bound passes; the algorithmic traffic is
20 bytes per element for SGD (read p, g, buf; write buf, p) and 28 for Adam (read p, g, m, v; write m, v, p).  Next to the ungrouped
SGD update, on the same arena and in the same alternation, the grouped one (dn_sgd_step_groups): "sgd_groups_split" with the network's
own 1x / 10x split (two runs), "sgd_groups_alternating" with the group changing on every slice (the most runs this arena can have).

    python tools/optimizer_bench.py [--launches 200] [--repeats 7] [--warmup 20]

Prints one JSON line: per optimizer the median / min / max time of a launch in microseconds and the achieved GB/s of the median."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args(argv)
    import torch
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench: needs an MI355X (there is no CPU path to time)")
    import bench
    import supervised_dispnet_amd.models as models
    from supervised_dispnet_amd import _lib, engine
    from supervised_dispnet_amd.optim import FusedAdam, FusedSGD, ParamArena, group_runs
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    bench._quiet_init(net)
    net.to(dev)
    arena = ParamArena(list(net._hot_parameters()), net._grad_production_order())
    arena.flat_g.normal_(0, 1e-3)
    opts = {"adam": (FusedAdam(arena, lr=1e-6), 28), "sgd": (FusedSGD(arena, lr=1e-6, momentum=0.9, weight_decay=5e-4), 20)}
    sgd = opts["sgd"][0]
    encoder = {id(p) for p in net.get_1x_lr_params()}
    tables = {"sgd_groups_split": [0 if id(p) in encoder else 1 for p in arena.params],
              "sgd_groups_alternating": [i % 2 for i in range(len(arena.params))]}
    rates = torch.tensor([1e-6, 1e-5], dtype=torch.float64, device=dev)
    runs_of = {}

    class Grouped(object):
        """dn_sgd_step_groups over the whole arena with one run table, on the ungrouped optimizer's buffers."""

        def __init__(self, group_of):
            self.runs = group_runs(arena.offsets, arena.numel, group_of)
            self.seg_end = torch.tensor([e for e, _ in self.runs], dtype=torch.int64, device=dev)
            self.seg_group = torch.tensor([g for _, g in self.runs], dtype=torch.int32, device=dev)

        def step(self):
            _lib.call("dn_sgd_step_groups", arena.flat_p.data_ptr(), arena.flat_g.data_ptr(), sgd.momentum_buffer.data_ptr(), 0, arena.numel,
                      self.seg_end.data_ptr(), self.seg_group.data_ptr(), len(self.runs), rates.data_ptr(), 2, 0.9, 5e-4, 1.0, engine._stream())

    for name, group_of in tables.items():
        opts[name] = (Grouped(group_of), 20)
        runs_of[name] = len(opts[name][0].runs)
    times = {k: [] for k in opts}
    for opt, _ in opts.values():
        for _ in range(args.warmup):
            opt.step()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name, (opt, _) in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                opt.step()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    assert bool(torch.isfinite(arena.flat_p).all())
    out = {"arena_elements": arena.numel, "launches_per_repeat": args.launches, "repeats": args.repeats}
    for name, (_, bytes_per) in opts.items():
        med = statistics.median(times[name])
        out[name] = {"us_median": round(med, 2), "us_min": round(min(times[name]), 2), "us_max": round(max(times[name]), 2),
                     "bytes_per_element": bytes_per, "GBps_median": round(arena.numel * bytes_per / med / 1e3, 1)}
        if name in runs_of:
            out[name]["runs"] = runs_of[name]
            out[name]["median_over_sgd"] = round(med / statistics.median(times["sgd"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
