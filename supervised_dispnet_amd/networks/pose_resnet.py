"""monodepth2's default pose network (`pose_model_type = separate_resnet`) on the HIP engine: the ResNet pair encoder
`ResnetEncoder(num_layers, pretrained, num_input_images=2)` followed by the reference's networks/pose_decoder.py `PoseDecoder(num_ch_enc,
num_input_features=1, num_frames_to_predict_for=2)`.  Every model monodepth2 publishes was trained with it: `pose_encoder.pth` is
`encoder.state_dict()` and `pose.pth` is `decoder.state_dict()` (keys `net.0.weight` .. `net.3.bias`), which load_monodepth2 /
save_monodepth2 read and write.

Forward contract = PoseCNN(2)'s: one [P, 6, H, W] tensor of stacked pairs in, `(axisangle, translation)` out, each [P, 1, 1, 3], views
of one dense [P, 6, 1, 1] tensor that rides on both as `._dn_pose_base` (loss_functions.monodepth2_loss / min_reprojection_loss read the
pose through it and hand its gradient back in one piece).  monodepth2's trainer reads only the FIRST predicted transform
(`axisangle[:, 0]`, `translation[:, 0]` in its predict_poses), so only rows 0..5 of `net.3` are evaluated: rows 6..11 are kept,
loaded and saved, and receive an exactly zero gradient.  A 12-wide base never reaches the loss, whose pose gradient is allocated for
exactly P * 6 elements.

Encoder and decoder run as ONE engine tape (run_net), as models.monodepth2 fuses its two halves: `encoder._hip_features`, then squeeze,
pose_0 and pose_1 as conv + ReLU, then engine.block_pose_tail -- `0.01 * mean_hw(conv1x1(x) + b)` as a spatial mean followed by a
[P, 256] x [256, 6] product, one launch per direction (csrc/dn_posetail.hip).  BatchNorm follows each module's own
`training` flag: batch statistics over the P pairs in train mode, frozen after `bn.eval()`.
"""
import os

import torch
import torch.nn as nn

from .. import engine
from .._lib import ACT_RELU
from ..models._common import run_net
from .resnet_encoder import ResnetEncoder

POSE_SCALE = 0.01


class PoseDecoderContainer(nn.Module):
    """Parameter container laid out like the reference's PoseDecoder: ModuleList `net` = squeeze, pose_0, pose_1, pose_2."""

    def __init__(self, num_ch_enc, num_input_features=1, num_frames_to_predict_for=2):
        super(PoseDecoderContainer, self).__init__()
        self.num_ch_enc = num_ch_enc
        self.num_input_features = num_input_features
        self.num_frames_to_predict_for = num_frames_to_predict_for
        self.net = nn.ModuleList([nn.Conv2d(int(num_ch_enc[-1]), 256, 1), nn.Conv2d(num_input_features * 256, 256, 3, 1, 1),
                                  nn.Conv2d(256, 256, 3, 1, 1), nn.Conv2d(256, 6 * num_frames_to_predict_for, 1)])


def _load_exact(module, state, what, optional_prefixes=()):
    """load_state_dict that names the offending key: every key and shape must match, except that `state` may lack keys under
    `optional_prefixes` (a monodepth2 pose_encoder.pth carries the unused `encoder.fc.*`; a checkpoint written without them loads too)."""
    own = module.state_dict()
    for k, v in state.items():                      # (shapes first: a PoseCNN pose.pth shares `net.0.weight` with PoseDecoder's)
        if k in own and tuple(v.shape) != tuple(own[k].shape):
            raise RuntimeError("%s: key '%s' has shape %s, %s expects %s" % (what, k, list(v.shape), type(module).__name__, list(own[k].shape)))
    for k in state:
        if k not in own:
            raise RuntimeError("%s: unexpected key '%s' (a %s state dict has %s ...)" % (what, k, type(module).__name__, ", ".join(list(own)[:3])))
    for k in own:
        if k not in state and not any(k.startswith(p) for p in optional_prefixes):
            raise RuntimeError("%s: missing key '%s'" % (what, k))
    module.load_state_dict(state, strict=False)


class PoseResnet(nn.Module):
    def __init__(self, num_layers=18, pretrained=False, num_frames_to_predict_for=2):
        super(PoseResnet, self).__init__()
        self.num_frames_to_predict_for = num_frames_to_predict_for
        self.encoder = ResnetEncoder(num_layers, pretrained, num_input_images=2)
        self.decoder = PoseDecoderContainer(self.encoder.num_ch_enc, 1, num_frames_to_predict_for)
        self._rt = None

    def forward(self, pairs):
        pose = run_net(self, pairs)[0]                             # [P, 6, 1, 1], dense: the first predicted transform
        v = pose.view(-1, 1, 1, 6)
        axisangle, translation = v[..., :3], v[..., 3:]
        axisangle._dn_pose_base = translation._dn_pose_base = pose
        return axisangle, translation

    def _hot_parameters(self):
        return list(self.encoder._hot_parameters()) + list(self.decoder.parameters())

    def _hip_forward(self, tape, sink, x):
        if self._rt is None:
            self._rt = [engine.ConvLayer(m) for m in self.decoder.net]
        rt = self._rt
        cur = self.encoder._hip_features(tape, sink, x)[-1]
        for layer in rt[:3]:
            cur = engine.block_conv_act(tape, sink, [engine.Piece(cur)], layer, ACT_RELU)
        return [engine.block_pose_tail(tape, sink, cur, rt[3], 6, POSE_SCALE)]

    # ---- monodepth2's two-file layout
    def load_monodepth2(self, folder):
        """`folder`/pose_encoder.pth + `folder`/pose.pth, bare state dicts with monodepth2's keys.  A missing `encoder.fc.*` is
        tolerated; any other mismatch is refused with the offending key in the message."""
        if not os.path.isdir(folder):
            raise RuntimeError("PoseResnet.load_monodepth2 takes a FOLDER holding pose_encoder.pth and pose.pth, got '%s'" % folder)
        dev = next(self.parameters()).device
        for name, module, optional in (("pose_encoder.pth", self.encoder, ("encoder.fc.",)), ("pose.pth", self.decoder, ())):
            path = os.path.join(folder, name)
            if not os.path.isfile(path):
                raise RuntimeError("PoseResnet.load_monodepth2: '%s' not found" % path)
            state = torch.load(path, map_location=dev)
            _load_exact(module, state.get("state_dict", state), path, optional)

    def save_monodepth2(self, folder):
        os.makedirs(folder, exist_ok=True)
        torch.save(self.encoder.state_dict(), os.path.join(folder, "pose_encoder.pth"))
        torch.save(self.decoder.state_dict(), os.path.join(folder, "pose.pth"))
