#!/usr/bin/env python3
"""Generate tests/golden/reproj.npz from the reference checkout: the outputs of its layers.py (transformation_from_parameters,
rot_from_axisangle, get_translation_matrix, BackprojectDepth, Project3D, and the minimum-reprojection composition of them with SSIM and
F.grid_sample) and of its networks/pose_cnn.py on the closed-form inputs of tests/reproj_audit.py.  Arrays only.

    DISPNET_REFERENCE=/path/to/reference python tests/golden/make_reproj_goldens.py

The reference's BackprojectDepth.forward stops in `pdb.set_trace()` without importing pdb: a no-op `pdb` is placed in the module's
namespace.
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

import reproj_audit as RA  # noqa: E402
from oracle import detgen  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, str(REF / rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _np(t):
    return t.detach().cpu().numpy()


def main():
    torch.set_num_threads(8)
    layers = _load("ref_layers", "layers.py")
    layers.pdb = types.SimpleNamespace(set_trace=lambda: None)
    pose_cnn = _load("ref_pose_cnn", "networks/pose_cnn.py")
    arrays = {}
    # ---- pose matrices
    aa, tr = RA.pose_vectors()
    arrays["pose:rot"] = _np(layers.rot_from_axisangle(aa))
    arrays["pose:trans"] = _np(layers.get_translation_matrix(tr))
    for inv in (False, True):
        a, t = aa.clone().requires_grad_(), tr.clone().requires_grad_()
        m = layers.transformation_from_parameters(a, t, invert=inv)
        (m * RA.pose_weight()).sum().backward()
        arrays["pose:M:inv%d" % inv], arrays["pose:daa:inv%d" % inv], arrays["pose:dt:inv%d" % inv] = _np(m), _np(a.grad), _np(t.grad)
    # ---- BackprojectDepth / Project3D
    for size in RA.GEOM_SIZES:
        h, w = size
        i = RA.geom_inputs(size)
        b = i["depth"].shape[0]
        depth, T = i["depth"].clone().requires_grad_(), i["T"].clone().requires_grad_()
        pts = layers.BackprojectDepth(b, h, w)(depth, i["inv_K"])
        (pts * i["gp"]).sum().backward()
        p = pts.detach().requires_grad_()
        grid = layers.Project3D(b, h, w)(p, i["K"], T)
        (grid * i["gg"]).sum().backward()
        tag = "geom:%dx%d:" % size
        arrays[tag + "points"], arrays[tag + "grid"], arrays[tag + "ddepth"], arrays[tag + "dT"] = _np(pts), _np(grid), _np(depth.grad), _np(T.grad)
        arrays[tag + "dpoints"] = _np(p.grad)
    # ---- the composition on the selection case
    name = "select_ragged"
    i = RA.inputs(name)
    b, _, h, w = i["tgt"].shape
    ssim = layers.SSIM()
    for ac in RA.ALIGNS:
        _, depth = layers.disp_to_depth(i["disp"], RA.MIN_DEPTH, RA.MAX_DEPTH)
        pts = layers.BackprojectDepth(b, h, w)(depth, i["inv_K"])
        ident, reproj = [], []
        for r, T in zip(i["refs"], i["T"]):
            pred = F.grid_sample(r, layers.Project3D(b, h, w)(pts, i["K"], T), mode="bilinear", padding_mode="border", align_corners=ac)
            reproj.append(RA.SSIM_W * ssim(pred, i["tgt"]).mean(1) + (1 - RA.SSIM_W) * (i["tgt"] - pred).abs().mean(1))
            ident.append(RA.SSIM_W * ssim(r, i["tgt"]).mean(1) + (1 - RA.SSIM_W) * (i["tgt"] - r).abs().mean(1))
        for am in RA.AUTOMASKS:
            m, sel = torch.stack((ident if am else []) + reproj, 1).min(1, keepdim=True)
            arrays["loss:%s:ac%d:am%d:m" % (name, ac, am)] = _np(m)
            arrays["loss:%s:ac%d:am%d:loss" % (name, ac, am)] = np.float64(m.mean().item())
    # ---- PoseCNN
    net = pose_cnn.PoseCNN(2)
    arrays["posecnn:keys"] = np.array(list(net.state_dict().keys()))
    net.load_state_dict(RA.pose_cnn_state())
    a, t = net(RA.pose_cnn_input())
    ga, gt = RA.pose_cnn_weights()
    ((a * ga).sum() + (t * gt).sum()).backward()
    arrays["posecnn:axisangle"], arrays["posecnn:translation"] = _np(a), _np(t)
    for k, p in net.named_parameters():
        for kk, v in detgen.summarize(p.grad, stride=53).items():
            arrays["posecnn:grad:%s:%s" % (k, kk)] = v
    out = HERE / "reproj.npz"
    np.savez_compressed(out, **arrays)
    print("wrote", out.name, "%.1f KB" % (out.stat().st_size / 1024))


if __name__ == "__main__":
    main()
