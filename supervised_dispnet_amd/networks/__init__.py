"""Mirror of the reference's `networks` package for the hot path (reference networks/__init__.py:1-5): the monodepth2-style
encoders / depth decoder and PoseCNN on the HIP engine, plus PoseResnet -- monodepth2's default pose network (`separate_resnet`: the
ResNet pair encoder followed by PoseDecoder's four convolutions), which the reference does not ship a trainer for but whose released
weights (`pose_encoder.pth` + `pose.pth`) it is meant to continue from.  PoseDecoder as a stand-alone module is dead code in the reference
(imported, never instantiated) and stays out of scope: its layout and arithmetic live in PoseResnet."""
from .depth_decoder import DepthDecoder
from .pose_cnn import PoseCNN
from .pose_resnet import PoseResnet
from .resnet_encoder import ResnetEncoder
from .vgg_encoder import vggEncoder


def _out_of_scope(name):
    class _Missing(object):
        def __init__(self, *a, **k):
            raise NotImplementedError("networks.%s is never instantiated by the reference (dead code) and is outside this build's scope; "
                                      "networks.PoseResnet holds its parameters (`.decoder`, a monodepth2 pose.pth) and runs it behind the "
                                      "pair encoder" % name)
    _Missing.__name__ = name
    return _Missing


PoseDecoder = _out_of_scope("PoseDecoder")


def _no_replication(self):
    """See supervised_dispnet_amd.models._no_replication: nn.DataParallel over ONE device works, replicas over several do not."""
    from ..models import _no_replication as f
    return f(self)


for _c in (DepthDecoder, ResnetEncoder, vggEncoder, PoseCNN, PoseResnet):
    _c._replicate_for_data_parallel = _no_replication
