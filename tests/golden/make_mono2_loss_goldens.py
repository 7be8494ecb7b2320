#!/usr/bin/env python3
"""Generate tests/golden/mono2_loss.npz from the reference checkout: monodepth2's multi-scale objective composed from the reference's
own layers.py (SSIM, get_smooth_loss, disp_to_depth, BackprojectDepth, Project3D) with F.interpolate and F.grid_sample, on the
ms_select case of tests/mono2_audit.py -- the per-scale parts and the total, for both align_corners values and both automask
settings.  It pins the restatement of tests/mono2_audit.py.  Arrays only.

    DISPNET_REFERENCE=/path/to/reference python tests/golden/make_mono2_loss_goldens.py
"""
import importlib.util
import os
import pathlib
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

if "DISPNET_REFERENCE" not in os.environ:
    raise SystemExit("set DISPNET_REFERENCE to the reference checkout")
REF = pathlib.Path(os.environ["DISPNET_REFERENCE"])
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import mono2_audit as MA  # noqa: E402
import reproj_audit as RA  # noqa: E402


def main():
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("ref_layers", str(REF / "layers.py"))
    layers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(layers)
    layers.pdb = types.SimpleNamespace(set_trace=lambda: None)
    name = "ms_select"
    i = MA.inputs(name)
    tgt = i["tgt"]
    b, _, h, w = tgt.shape
    ssim = layers.SSIM()
    term = lambda pred: RA.SSIM_W * ssim(pred, tgt).mean(1) + (1 - RA.SSIM_W) * (tgt - pred).abs().mean(1)
    arrays = {}
    for ac in MA.ALIGNS:
        for am in MA.AUTOMASKS:
            parts, total = [], 0.0
            for s, d in enumerate(i["disps"]):
                up = d if s == 0 else F.interpolate(d, (h, w), mode="bilinear", align_corners=False)
                _, depth = layers.disp_to_depth(up, RA.MIN_DEPTH, RA.MAX_DEPTH)
                pts = layers.BackprojectDepth(b, h, w)(depth, i["inv_K"])
                ident, reproj = [], []
                for r, T in zip(i["refs"], i["T"]):
                    grid = layers.Project3D(b, h, w)(pts, i["K"], T)
                    reproj.append(term(F.grid_sample(r, grid, mode="bilinear", padding_mode="border", align_corners=ac)))
                    ident.append(term(r))
                m = torch.stack((ident if am else []) + reproj, 1).min(1)[0]
                norm = d / (d.mean(2, True).mean(3, True) + 1e-7)
                colour = tgt if s == 0 else F.interpolate(tgt, (h >> s, w >> s), mode="area")
                sm = layers.get_smooth_loss(norm, colour)
                parts.append([m.mean().item(), sm.item()])
                total += m.mean().item() + MA.SMOOTHNESS / 2 ** s * sm.item()
            arrays["%s:ac%d:am%d:parts" % (name, ac, am)] = np.array(parts, dtype=np.float64)
            arrays["%s:ac%d:am%d:loss" % (name, ac, am)] = np.float64(total / len(parts))
    out = HERE / "mono2_loss.npz"
    np.savez_compressed(out, **arrays)
    print("wrote", out.name, "%.1f KB" % (out.stat().st_size / 1024))


if __name__ == "__main__":
    main()
