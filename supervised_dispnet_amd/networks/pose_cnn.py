"""Mirror of the reference's networks/pose_cnn.py (monodepth2's PoseCNN) on the HIP engine.

Constructor `PoseCNN(num_input_frames)`, state_dict keys (`net.0.weight` .. `net.6.bias`, `pose_conv.*`: a monodepth2 `pose.pth`
loads) and the forward contract -- one [B, 3N, H, W] tensor in, `(axisangle, translation)` out, each [B, N-1, 1, 3] -- follow
reference networks/pose_cnn.py:13-50.  The layer stack is models.PoseExpNet's encoder and runs the same way: seven stride-2
convolutions with the ReLU in their epilogue, the 1x1 `pose_conv`, and `0.01 * mean_hw` as one reduction kernel.

The two results are views of one dense [B, N-1, 6] tensor, which rides on both as `._dn_pose_base`:
loss_functions.min_reprojection_loss reads the pose through it and hands its gradient back in one piece, so that no framework
kernel (the slices' backward) sits between the network and the loss and a whole step can go on a graph.TapedStep.
"""
import torch.nn as nn

from .. import engine
from .._lib import ACT_NONE, ACT_RELU
from ..models._common import run_net

_PLANES = (16, 32, 64, 128, 256, 256, 256)
_KERNELS = (7, 5, 3, 3, 3, 3, 3)


class PoseCNN(nn.Module):
    def __init__(self, num_input_frames):
        super(PoseCNN, self).__init__()
        self.num_input_frames = num_input_frames
        convs, c_in = [], 3 * num_input_frames
        for c_out, k in zip(_PLANES, _KERNELS):
            convs.append(nn.Conv2d(c_in, c_out, k, 2, (k - 1) // 2))
            c_in = c_out
        self.pose_conv = nn.Conv2d(c_in, 6 * (num_input_frames - 1), 1)
        self.num_convs = len(convs)
        self.relu = nn.ReLU(True)
        self.net = nn.ModuleList(convs)
        self._rt = None

    def forward(self, out):
        pose = run_net(self, out)[0]                               # [B, 6 (N-1), 1, 1], dense
        v = pose.view(-1, self.num_input_frames - 1, 1, 6)
        axisangle, translation = v[..., :3], v[..., 3:]
        axisangle._dn_pose_base = translation._dn_pose_base = pose
        return axisangle, translation

    def _hot_parameters(self):
        return list(self.parameters())

    def _runtime(self):
        if self._rt is None:
            self._rt = [engine.ConvLayer(m) for m in self.net] + [engine.ConvLayer(self.pose_conv)]
        return self._rt

    def _hip_forward(self, tape, sink, x):
        rt = self._runtime()
        cur = x
        for layer in rt[:-1]:
            cur = engine.block_conv_act(tape, sink, [engine.Piece(cur)], layer, ACT_RELU)
        pose_map = engine.block_conv_act(tape, sink, [engine.Piece(cur)], rt[-1], ACT_NONE)
        return [engine.block_spatial_mean(tape, pose_map, 0.01)]
