#!/usr/bin/env python3
"""Can the NYU Depth v2 loader keep one MI355X fed?  Fabricates a tree of (5, 320, 448) float32 samples in a temporary directory and
reports, as one JSON line:

  loader_only_img_s      NyuLoader (reader threads -> pinned staging -> H2D on a side stream -> dn_nyu_prefilter +
                         dn_nyu_train_resample) iterated flat out at -b
  kernel_ms_per_batch    the two training kernels on a device-resident batch (HIP events), and each of them alone
  val_resize_ms_per_batch dn_nyu_val_resize of a [B,3,480,640] batch
  train_resident_img_s   the Disp_vgg_BN L1 training step at 256x352 on a resident batch -- what train.py --synthetic --dataset nyu
                         --img-height 256 --img-width 352 runs per step
  train_nyu_img_s        the same step fed by the NyuLoader

usage: python tools/nyu_loader_bench.py [--files 128] [--batch 32] [--steps 20] [--readers 16]"""
import argparse, json, os, pathlib, shutil, sys, tempfile, time
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--files", type=int, default=128)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--readers", type=int, default=16)
a = ap.parse_args()

import __graft_entry__
__graft_entry__.build(only_library=True)
import bench
import supervised_dispnet_amd.loss_functions as LF
import supervised_dispnet_amd.models as models
from supervised_dispnet_amd import _lib, nyu
from supervised_dispnet_amd.functional import reciprocal
from supervised_dispnet_amd.optim import FusedAdam

dev = torch.device("cuda:0")
B, H0, W0 = a.batch, 320, 448
th, tw = nyu.TRAIN_SIZE
tmp = tempfile.mkdtemp(prefix="dn_nyu_")
try:
    r = np.random.RandomState(0)
    tdir = nyu.train_dir(tmp)
    os.makedirs(tdir)
    for i in range(a.files):
        rgb = r.randint(0, 256, (3, H0, W0)).astype(np.float32)
        mask = (r.rand(1, H0, W0) < 0.9).astype(np.float32)
        np.save(os.path.join(tdir, "%05d.npy" % i), np.concatenate([rgb, (0.5 + 9.5 * r.rand(1, H0, W0)).astype(np.float32) * mask, mask]))
    out = {"files": a.files, "batch": B, "raw": [5, H0, W0], "crop": [th, tw], "readers": a.readers}

    def rate(it, steps, per=B):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        for _ in it:
            k += 1
            if k == steps:
                break
        torch.cuda.synchronize()
        return k * per / (time.perf_counter() - t0)

    loader = nyu.NyuLoader(tmp, B, dev, train=True, seed=0, readers=a.readers)

    def loop():
        e = 0
        while True:
            loader.set_epoch(e)
            for b in loader:
                yield b
            e += 1

    rate(loop(), 3)
    out["loader_only_img_s"] = rate(loop(), a.steps)

    def timed(fn, reps=20):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    raw = torch.from_numpy(np.stack([nyu.NyuTrainSet(tmp)[i % a.files] for i in range(B)])).to(dev)
    par = torch.from_numpy(nyu.params_array([nyu.draw_params(np.random.RandomState(i), H0, W0) for i in range(B)])).to(dev)
    coef, mm = nyu.new_workspace(B, H0, W0, dev)
    img = torch.empty((B, 3, th, tw), device=dev)
    dep = torch.empty((B, th, tw), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pre = lambda: _lib.call("dn_nyu_prefilter", raw.data_ptr(), par.data_ptr(), B, H0, W0, coef.data_ptr(), mm.data_ptr(), st)  # noqa: E731
    res = lambda: _lib.call("dn_nyu_train_resample", coef.data_ptr(), mm.data_ptr(), par.data_ptr(), B, H0, W0, th, tw, nyu._MEAN_H,  # noqa: E731
                            nyu._STD_H, img.data_ptr(), dep.data_ptr(), st)
    out["prefilter_ms_per_batch"] = timed(pre)
    out["resample_ms_per_batch"] = timed(res)
    out["kernel_ms_per_batch"] = timed(lambda: (pre(), res()))
    vimg = torch.rand((B, 3, 480, 640), device=dev) * 255
    out["val_resize_ms_per_batch"] = timed(lambda: nyu.resize_batch(vimg))
    del raw, coef, vimg

    torch.manual_seed(0)
    net = models.Disp_vgg_BN(datasets="nyu", with_classifier=False)
    bench._quiet_init(net)
    net.to(dev).train()
    opt = FusedAdam(net._hot_parameters(), lr=1e-4, production_order=net._grad_production_order())

    def step(x, gt):
        depth = [reciprocal(d) for d in net(x)]
        loss = LF.l1_loss(gt, depth, "nyu")
        opt.zero_grad()
        loss.backward()
        opt.step()

    x0, g0 = img.clone(), dep.clone()
    for _ in range(3):
        step(x0, g0)

    def resident():
        while True:
            step(x0, g0)
            yield None

    def fed():
        for x, gt in loop():
            step(x, gt)
            yield None

    out["train_resident_img_s"] = rate(resident(), a.steps)
    rate(fed(), 3)
    out["train_nyu_img_s"] = rate(fed(), a.steps)
    out["train_nyu_over_resident"] = out["train_nyu_img_s"] / out["train_resident_img_s"]
    out["loader_keeps_up"] = out["loader_only_img_s"] >= out["train_resident_img_s"]
    print(json.dumps(out))
finally:
    shutil.rmtree(tmp, ignore_errors=True)
