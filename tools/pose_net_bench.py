#!/usr/bin/env python3
"""What monodepth2's ResNet pose network (networks.PoseResnet) costs, in ONE process.

    python tools/pose_net_bench.py [--repeats 5] [--window-s 0.5] [--skip-step] [--out FILE.json]

(a) the fused pose tail (engine.block_pose_tail: dn_pose_tail_fwd / _bwd) against the route composed from the blocks that existed before
    it (block_conv_act with ACT_NONE over all 12 rows, then block_spatial_mean), forward + backward, at P = 24 pairs on the 4 x 13 and
    the 6 x 20 map: launches per forward + backward and the time of one taped replay of them;
(b) PoseCNN against PoseResnet, forward + backward, at 24 x 6 x 128 x 416;
(c) the whole taped training step of disp_res_18 + monodepth2_loss + fused Adam at 12 images (two source frames: 24 pairs) with each
    pose model;
(d) per layer of the pair encoder, forward and backward: the kernel that ran and its time between two HIP events in an eager step
    (this includes the launch itself; it says which kernel family a layer lands on -- the 6-channel 7 x 7 stem in particular -- and
    roughly what it costs, not more).

Everything in (a)-(c) is recorded on a launch tape (graph.TapedStep) and the candidates are timed ALTERNATELY, `repeats` windows each:
a window is warmed, replays until `window-s` seconds have passed and ends in a device synchronise (host clock around it).  Printed per
candidate: every window, the median, and the spread (max - min) between windows of the SAME candidate -- the yardstick a difference has
to beat.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def alternate(cands, repeats, seconds):
    """cands: {name: TapedStep} -> {name: dict(us=[...], median_us, spread_us, launches)}"""
    times = {k: [] for k in cands}
    for _ in range(repeats):
        for k, ts in cands.items():
            times[k].append(1e6 * window(ts, seconds))
    out = {}
    for k, ts in cands.items():
        us = times[k]
        out[k] = {"us": [round(v, 2) for v in us], "median_us": round(statistics.median(us), 2), "spread_us": round(max(us) - min(us), 2),
                  "launches": int(ts.launches), "fences": int(ts.fences)}
        print("  %-22s median %10.2f us  spread %8.2f us  launches %4d  (%s)" % (k, out[k]["median_us"], out[k]["spread_us"], ts.launches,
                                                                                 " ".join("%.2f" % v for v in us)), flush=True)
    return out


class _Tail(nn.Module):
    """pose_2 of the decoder on a given activation: fused, or composed from the conv and mean blocks"""

    def __init__(self, fused):
        super().__init__()
        self.conv = nn.Conv2d(256, 12, 1)
        self.fused, self._rt = fused, None

    def _hot_parameters(self):
        return list(self.parameters())

    def _hip_forward(self, tape, sink, x):
        from supervised_dispnet_amd import engine
        from supervised_dispnet_amd._lib import ACT_NONE
        if self._rt is None:
            self._rt = engine.ConvLayer(self.conv)
        if self.fused:
            return [engine.block_pose_tail(tape, sink, x, self._rt, 6, 0.01)]
        return [engine.block_spatial_mean(tape, engine.block_conv_act(tape, sink, [engine.Piece(x)], self._rt, ACT_NONE), 0.01)]


def fwd_bwd_tape(net, x, run):
    """TapedStep of `run(net, x)` -> the tensor to differentiate, and its backward; gradients are dropped each step so that autograd
    assigns (no framework accumulation kernel)"""
    from supervised_dispnet_amd.graph import TapedStep, backward
    params = list(net.parameters())

    def step():
        for p in params:
            p.grad = None
        x.grad = None
        out = run(net, x)
        backward(out)
        return out

    return TapedStep(step, warmup=2, static_inputs=(x,)).capture()


def tail_section(dev, args):
    from supervised_dispnet_amd.models._common import run_net
    res = {}
    for h, w in ((4, 13), (6, 20)):
        torch.manual_seed(0)
        x = torch.rand(24, 256, h, w, device=dev).relu_().contiguous(memory_format=torch.channels_last).requires_grad_()
        nets = {"fused": _Tail(True).to(dev), "composed": _Tail(False).to(dev)}
        nets["composed"].load_state_dict(nets["fused"].state_dict())
        tapes = {k: fwd_bwd_tape(n, x, lambda n, x: run_net(n, x)[0]) for k, n in nets.items()}
        a, b = tapes["fused"].out.detach().flatten(1), tapes["composed"].out.detach().flatten(1)[:, :6]
        print("(a) pose tail, P 24, HW %d (%d x %d): fused against composed, max |difference| of the outputs %.3g" % (
            h * w, h, w, float((a - b).abs().max())), flush=True)
        res["HW%d" % (h * w)] = alternate(tapes, args.repeats, args.window_s)
        for t in tapes.values():
            t.close()
    return res


def pose_section(dev, args):
    import supervised_dispnet_amd.networks as networks
    torch.manual_seed(0)
    x = torch.rand(24, 6, 128, 416, device=dev)
    nets = {"PoseCNN": networks.PoseCNN(2).to(dev).train(), "PoseResnet": networks.PoseResnet(18).to(dev).train()}
    tapes = {k: fwd_bwd_tape(n, x, lambda n, x: n(x)[0]._dn_pose_base) for k, n in nets.items()}
    print("(b) pose networks, forward + backward, 24 x 6 x 128 x 416", flush=True)
    res = alternate(tapes, args.repeats, args.window_s)
    for t in tapes.values():
        t.close()
    return res, nets["PoseResnet"], x


def step_section(dev, args):
    import supervised_dispnet_amd.loss_functions as LF
    import supervised_dispnet_amd.models as models
    import supervised_dispnet_amd.networks as networks
    from supervised_dispnet_amd.graph import TapedStep, backward
    from supervised_dispnet_amd.optim import FusedAdam
    B, H, W, F = 12, 128, 416, 2
    torch.manual_seed(0)
    tgt = torch.rand(B, 3, H, W, device=dev)
    refs = [(tgt + 0.05 * torch.rand(B, 3, H, W, device=dev)).clamp_(0, 1) for _ in range(F)]
    earlier = [f < F // 2 for f in range(F)]
    pairs = torch.cat([torch.cat([r, tgt] if e else [tgt, r], 1) for r, e in zip(refs, earlier)], 0)
    K = torch.eye(4).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    Kinv = torch.inverse(K).contiguous().to(dev)          # (torch.inverse hands back column-major matrices; the loss reads dense ones)
    K = K.contiguous().to(dev)
    tapes, keep = {}, []
    for name in ("posecnn", "resnet18"):
        torch.manual_seed(1)
        enc = networks.ResnetEncoder(18, False)
        depth_net = models.monodepth2(enc, networks.DepthDecoder(enc.num_ch_enc)).to(dev).train()
        pose_net = (networks.PoseCNN(2) if name == "posecnn" else networks.PoseResnet(18)).to(dev).train()
        opt = FusedAdam(list(depth_net._hot_parameters()) + list(pose_net._hot_parameters()), lr=1e-4)

        def step(depth_net=depth_net, pose_net=pose_net, opt=opt):
            base = pose_net(pairs)[0]._dn_pose_base
            v = base.view(F, B, 1, 6).permute(1, 0, 2, 3)
            aa, tr = v[..., :3], v[..., 3:]
            aa._dn_pose_base = tr._dn_pose_base = base
            loss = LF.monodepth2_loss(tgt, refs, depth_net(tgt), K, Kinv, (aa, tr, earlier), scaled_disp=True, smoothness=1e-3)
            opt.zero_grad()
            backward(loss)
            opt.step()
            return loss

        tapes[name] = TapedStep(step, optimizer=opt, warmup=2, static_inputs=(tgt, pairs) + tuple(refs)).capture()
        keep.append((depth_net, pose_net, opt))
    print("(c) taped training step, disp_res_18 + monodepth2_loss + fused Adam, 12 images, 24 pairs", flush=True)
    res = alternate(tapes, args.repeats, args.window_s)
    for t in tapes.values():
        t.close()
    return res


def layer_section(net, x):
    """eager forward + backward of PoseResnet with the engine's per-launch events on: (kernel, what, microseconds) per recorded launch"""
    from supervised_dispnet_amd import engine
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        net(x)[0]._dn_pose_base.sum().backward()
    torch.cuda.synchronize()
    for p in net.parameters():
        p.grad = None
    engine.PROFILE = []
    try:
        net(x)[0]._dn_pose_base.sum().backward()
        torch.cuda.synchronize()
        rows = [(r[0], r[4], 1e3 * r[2].elapsed_time(r[3])) for r in engine.PROFILE]
    finally:
        engine.PROFILE = None
    print("(d) PoseResnet, 24 x 6 x 128 x 416, one eager forward + backward: kernel per recorded launch (us between two events)", flush=True)
    for kernel, what, us in rows:
        print("  %9.1f us  %-46s %s" % (us, what, kernel), flush=True)
    return [{"kernel": k, "what": w, "us": round(u, 1)} for k, w, u in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--skip-step", action="store_true", help="leave out (c), the whole training step")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_net_bench: needs the GPU (no fallback: a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    result = {"tool": "pose_net_bench", "device": torch.cuda.get_device_name(0), "window_s": args.window_s, "repeats": args.repeats}
    result["tail"] = tail_section(dev, args)
    result["pose_networks"], net, x = pose_section(dev, args)
    result["encoder_layers"] = layer_section(net, x)
    del net, x
    if not args.skip_step:
        result["training_step"] = step_section(dev, args)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
