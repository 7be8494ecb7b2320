#!/usr/bin/env python3
"""Generate tests/golden/pose_resnet.npz from the reference checkout: its networks/pose_decoder.py `PoseDecoder([64,64,128,256,512], 1, 2)`
and its networks/resnet_encoder.py `ResnetEncoder(18, False, 2)` on the closed-form inputs of tests/pose_net_audit.py.  Arrays only.

    DISPNET_REFERENCE=/path/to/reference python tests/golden/make_pose_resnet_goldens.py

The pair encoder subclasses torchvision.models.ResNet; torchvision only contributes the layout, which the shim of make_goldens.py
provides (imported, not edited).
"""
import os
import pathlib
import sys

import numpy as np
import torch

if "DISPNET_REFERENCE" not in os.environ:
    raise SystemExit("set DISPNET_REFERENCE to the reference checkout")
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import make_goldens as MG  # noqa: E402  (reads DISPNET_REFERENCE itself)
import pose_net_audit as PA  # noqa: E402
from oracle import detgen  # noqa: E402


def _np(t):
    return t.detach().cpu().numpy()


def main():
    torch.set_num_threads(8)
    MG._install_shims()
    ref_dec = MG._load("ref_pose_decoder", "networks/pose_decoder.py")
    ref_enc = MG._load("ref_resnet_encoder", "networks/resnet_encoder.py")
    arrays = {}
    ga, gt = PA.out_weights()

    def first_transform_loss(aa, tr):                       # what monodepth2's trainer reads
        return (aa[:, :1] * ga).sum() + (tr[:, :1] * gt).sum()

    # ---- PoseDecoder alone
    dec = ref_dec.PoseDecoder(np.array([64, 64, 128, 256, 512]), 1, 2)
    arrays["dec:keys"] = np.array(list(dec.state_dict().keys()))
    for k, v in dec.state_dict().items():
        arrays["dec:shape:" + k] = np.array(v.shape, dtype=np.int64)
    dec.load_state_dict(PA.decoder_state())
    aa, tr = dec([[PA.decoder_feature()]])
    first_transform_loss(aa, tr).backward()
    arrays["dec:axisangle"], arrays["dec:translation"] = _np(aa), _np(tr)
    for k, p in dec.named_parameters():
        for kk, v in detgen.summarize(p.grad, stride=PA.grad_stride(p.numel())).items():
            arrays["dec:grad:%s:%s" % (k, kk)] = v
    # ---- the pair encoder in train mode, and the decoder behind it
    enc = ref_enc.ResnetEncoder(18, False, 2)
    arrays["enc:keys"] = np.array(list(enc.state_dict().keys()))
    for k, v in enc.state_dict().items():
        arrays["enc:shape:" + k] = np.array(v.shape, dtype=np.int64)
    enc.load_state_dict(PA.encoder_state())
    enc.train()
    dec.zero_grad()
    feats = enc(PA.net_input())
    for kk, v in detgen.summarize(feats[-1], stride=53).items():
        arrays["enc:last:" + kk] = v
    aa, tr = dec([feats])
    first_transform_loss(aa, tr).backward()
    arrays["net:axisangle"], arrays["net:translation"] = _np(aa), _np(tr)
    out = HERE / "pose_resnet.npz"
    np.savez_compressed(out, **arrays)
    print("wrote", out.name, "%.1f KB" % (out.stat().st_size / 1024))


if __name__ == "__main__":
    main()
