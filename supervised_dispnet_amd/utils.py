"""Mirror of the hot-path pieces of the reference's utils.py: the SID discretisation used by the DORN head / loss, and tensor2array,
the host statement of the colouring run_inference.py writes (the device form is dn_colorize_u8, supervised_dispnet_amd/inference.py)."""
import os

import numpy as np
import torch

from . import _lib
from .engine import _stream, require_cuda


def _beta(dataset):
    if dataset == 'kitti':
        return 80.999
    if dataset in ('nyu', 'NYU'):
        return 10.999
    raise ValueError("undefined dataset %r" % (dataset,))


@torch.no_grad()
def get_labels_sid(depth, ordinal_c=71.0, dataset='kitti'):
    """reference utils.py:147-175: int32 labels = int(K * log(depth + 0.999) / log(beta)) (truncation toward zero)."""
    require_cuda(depth, "depth")
    if dataset == 'NYU':
        raise UnboundLocalError("get_labels_sid only knows 'kitti' and 'nyu' (reference utils.py:153-158)")
    d = depth.contiguous().float()
    out = torch.empty(d.shape, dtype=torch.int32, device=d.device)
    _lib.call("dn_sid_labels", d.data_ptr(), d.numel(), float(ordinal_c), _beta(dataset), out.data_ptr(), _stream())
    return out


@torch.no_grad()
def get_depth_sid(labels, ordinal_c=71.0, dataset='kitti'):
    """reference utils.py:106-133: 0.5 * (beta^(l/K) + beta^((l+1)/K)) - 0.999."""
    require_cuda(labels, "labels")
    l = labels.contiguous().to(torch.int64)
    out = torch.empty(l.shape, dtype=torch.float32, device=l.device)
    _lib.call("dn_sid_depth", l.data_ptr(), l.numel(), float(ordinal_c), _beta(dataset), out.data_ptr(), _stream())
    return out


def colour_table(colormap):
    """OpenCV's colour map as uint8 [256, 3] RGB -- cv2.applyColorMap is a per-value lookup, so colouring arange(256) is the whole map --
    or None when cv2 does not import (tensor2array then takes the reference's grey branch).  The tables are OpenCV's own data: they
    are read from it, not restated here."""
    try:
        import cv2
    except ImportError:
        return None
    code = {"rainbow": cv2.COLORMAP_RAINBOW, "bone": cv2.COLORMAP_BONE}[colormap]
    bgr = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), code)
    return np.ascontiguousarray(bgr[:, 0, ::-1])


def tensor2array(tensor, max_value=255, colormap='rainbow', channel_first=True, table=None):
    """reference utils.py:45-76.  A 2-D map or one with a leading dimension of 1 is divided by max_value (None: its own maximum) and
    coloured: through `table` (uint8 [256, 3] RGB; default OpenCV's `colormap`) at index uint8(clip(255 * x / max_value, 0, 255)), or,
    without OpenCV and without a table, as grey clip(x / max_value, 0, 1) in three channels -- the reference's ImportError branch, which
    only takes 2-D maps there ([1, h, w] is squeezed here as in the table branch).  A [3, h, w] tensor is 0.5 + 0.5 * x.  float32 in
    [0, 1], [3, h, w] or, with channel_first=False, [h, w, 3]."""
    tensor = tensor.detach().cpu()
    if max_value is None:
        max_value = tensor.max().item()
    if tensor.ndimension() == 2 or tensor.size(0) == 1:
        if table is None:
            table = colour_table(colormap)
        plane = tensor.squeeze().numpy()
        if table is not None:
            index = (255 * plane / max_value).clip(0, 255).astype(np.uint8)
            array = np.asarray(table, dtype=np.uint8)[index].astype(np.float32) / 255
        else:
            array = (np.repeat(plane[:, :, None], 3, axis=2) / max_value).clip(0, 1)
        if channel_first:
            array = array.transpose(2, 0, 1)
    elif tensor.ndimension() == 3:
        assert tensor.size(0) == 3
        array = 0.5 + tensor.numpy() * 0.5
        if not channel_first:
            array = array.transpose(1, 2, 0)
    return array


def load_model(pretrained_model, weights_folder):
    """Monodepth2 weight loader of the reference (train.py:726-751, test_disp.py:85-86): for n in ("encoder", "depth") read
    <weights_folder>/<n>.pth, keep the keys the module has, load.  Fails loudly when the folder or a file is missing."""
    folder = os.path.expanduser(weights_folder) if weights_folder else weights_folder
    if not folder or not os.path.isdir(folder):
        raise FileNotFoundError("Cannot find folder {}".format(folder))
    print("loading model from folder {}".format(folder))
    for n in ("encoder", "depth"):
        print("Loading {} weights...".format(n))
        path = os.path.join(folder, "{}.pth".format(n))
        model_dict = pretrained_model[n].state_dict()
        pretrained_dict = torch.load(path, map_location="cpu")
        model_dict.update({k: v for k, v in pretrained_dict.items() if k in model_dict})
        pretrained_model[n].load_state_dict(model_dict)
