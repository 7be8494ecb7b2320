#!/usr/bin/env python3
"""Generate tests/golden/nyu_transform.npz by running the REFERENCE's own NYU transform chain (build container only).

    python tests/golden/make_nyu_goldens.py        # DISPNET_REFERENCE=<path> overrides the default reference location

The reference's datasets/image_utils.py and datasets/nyu_depth_v2.py are imported as they are; what this container lacks is shimmed:
  * collections.Sequence -> collections.abc.Sequence (removed in Python 3.10);
  * torchvision.transforms ToTensor / Normalize / Lambda and torchvision.utils: ToTensor = HWC -> CHW torch.from_numpy, divided by 255
    for uint8 input only (so the float arrays here are NOT divided); Normalize = (t - mean) / std with mean / std as tensors of t's dtype;
    Lambda = call the function;
  * numpy >= 1.23 refuses the list-of-slices index of the reference's Split: Split receives its array as a view that accepts it
    (_ListIndexable), Split's own code runs unchanged;
  * skimage.transform.warp / AffineTransform (skimage is not installed).  AffineTransform(scale=(s, s)) holds diag(s, s, 1) and
    `.inverse` the transform of np.linalg.inv of it; warp(image, tf) is restated as bilinear (order=1) per channel, cval 0 outside the
    image, clipped to the input's [min, max] (clip=True), float64 output -- tests/nyu_chain.warp_scale, which follows skimage's
    bilinear formula.  Only pure scale transforms are accepted.
Inputs are formulas (tests/nyu_chain.raw_sample / raw_test_images / raw_test_depths); the file stores the draws (recorded from the
reference's own random calls) and the outputs -- of the full-size case every 16th row and the last (`full_rows`), to keep the
fixture small.  Nothing of the reference's source is copied.
"""
import collections
import collections.abc
import importlib.util
import os
import pathlib
import sys
import types

import numpy as np
import torch

REF = pathlib.Path(os.environ.get("DISPNET_REFERENCE", "/root/reference"))
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import nyu_chain  # noqa: E402

OUT = HERE / "nyu_transform.npz"


class _ListIndexable(np.ndarray):
    """The reference's Split indexes with a LIST of slices, which numpy >= 1.23 refuses; the array Split receives
    takes such a list as the tuple older numpy took it for.  Values are untouched."""

    def __getitem__(self, idx):
        return super().__getitem__(tuple(idx) if isinstance(idx, list) else idx)


def _install_shims():
    if not hasattr(collections, "Sequence"):
        collections.Sequence = collections.abc.Sequence
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvu = types.ModuleType("torchvision.utils")

    class ToTensor(object):
        def __call__(self, pic):
            t = torch.from_numpy(np.ascontiguousarray(pic.transpose((2, 0, 1))))
            return t.float().div(255) if t.dtype == torch.uint8 else t

    class Normalize(object):
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, t):
            m = torch.as_tensor(self.mean, dtype=t.dtype)[:, None, None]
            s = torch.as_tensor(self.std, dtype=t.dtype)[:, None, None]
            return t.sub(m).div(s)

    class Lambda(object):
        def __init__(self, fn):
            self.fn = fn

        def __call__(self, x):
            return self.fn(x)

    tvt.ToTensor, tvt.Normalize, tvt.Lambda = ToTensor, Normalize, Lambda
    tv.transforms, tv.utils = tvt, tvu
    sk = types.ModuleType("skimage")
    skt = types.ModuleType("skimage.transform")

    class AffineTransform(object):
        def __init__(self, scale=(1.0, 1.0), matrix=None):
            self.params = np.array(matrix, dtype=np.float64) if matrix is not None else np.diag([scale[0], scale[1], 1.0])

        @property
        def inverse(self):
            return AffineTransform(matrix=np.linalg.inv(self.params))

    def warp(image, inverse_map):
        M = inverse_map.params
        assert M[0, 0] == M[1, 1] and not M[0, 1] and not M[1, 0] and not M[0, 2] and not M[1, 2], "only pure scales are restated"
        return nyu_chain.warp_scale(image, M[0, 0])

    skt.warp, skt.AffineTransform = warp, AffineTransform
    sk.transform = skt
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.utils": tvu, "skimage": sk, "skimage.transform": skt})


def _load_reference():
    _install_shims()
    pkg = types.ModuleType("refdatasets")
    pkg.__path__ = [str(REF / "datasets")]
    sys.modules["refdatasets"] = pkg
    mods = {}
    for name in ("image_utils", "nyu_depth_v2"):
        spec = importlib.util.spec_from_file_location("refdatasets." + name, REF / "datasets" / (name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["refdatasets." + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
        if name == "image_utils":
            split_call = m.Split.__call__
            m.Split.__call__ = lambda self, image: split_call(self, np.asarray(image).view(_ListIndexable))
    return mods["nyu_depth_v2"]


class _Recorder(object):
    """Stands in for np.random inside the reference's transforms and records every draw."""

    def __init__(self):
        self.log = []

    def uniform(self, *a):
        v = np.random.uniform(*a)
        self.log.append(float(v))
        return v

    def randint(self, *a):
        v = np.random.randint(*a)
        self.log.append(int(v))
        return v


def _train_case(N, raw, k, size):
    tf = N.NYU_Depth_V2.get_transform(training=True, size=size)
    rec = _Recorder()
    for t in tf.transforms:
        if hasattr(t, "random_state"):
            t.random_state = rec
        elif isinstance(t, list):
            for u in t:
                if hasattr(u, "random_state"):
                    u.random_state = rec
    np.random.seed(k)
    img, depth = N.transform_chw(tf, [raw[0:3], raw[3:5]])
    log = rec.log
    log_next = np.random.uniform()                      # where the reference leaves the global stream: pins the draw count
    if len(log) == 4:                                   # exact size: flip, angle, zoom, colour (no crop draws)
        draws = (log[0] > 0.5, log[1], 0, 0, log[2], log[3])
    else:                                               # flip, angle, crop row, crop column, zoom, colour
        draws = (log[0] > 0.5, log[1], log[2], log[3], log[4], log[5])
    assert img.dtype == torch.float32 and depth.dtype == torch.float32
    return img.numpy(), depth.numpy()[0], np.asarray(draws, dtype=np.float64), len(log), log_next


def main():
    N = _load_reference()
    out = {}
    cases = [("small", 44, 60, (32, 48), [0, 1, 2, 3]), ("exact", 32, 48, (32, 48), [4, 5]), ("full", 320, 448, (256, 352), [6])]
    for name, H0, W0, size, seeds in cases:
        raws = np.stack([nyu_chain.raw_sample(H0, W0, "nyu:%s:%d" % (name, k)) for k in seeds])
        imgs, deps, draws, counts, nexts = [], [], [], [], []
        for j, k in enumerate(seeds):
            i, d, p, n, x = _train_case(N, raws[j], k, size)
            imgs.append(i)
            deps.append(d)
            draws.append(p)
            counts.append(n)
            nexts.append(x)
        # the full-size case keeps every 16th output row and the last one (the whole 256x352 output would be 1.4 MB of fixture)
        rows = np.r_[0:size[0]:16, size[0] - 1] if name == "full" else np.arange(size[0])
        out[name + "_rows"] = rows
        out[name + "_img"] = np.stack(imgs)[:, :, rows]
        out[name + "_depth"] = np.stack(deps)[:, rows]
        out[name + "_draws"] = np.stack(draws)
        out[name + "_ndraws"] = np.asarray(counts)
        out[name + "_next"] = np.asarray(nexts)
        out[name + "_seeds"] = np.asarray(seeds)
        out[name + "_shape"] = np.asarray([H0, W0, size[0], size[1]])
    # validation: BilinearResize(320/480, 448/640) of a smaller image (the same factors) keeps the fixture small
    ims = nyu_chain.raw_test_images(2, "nyu:val", 60, 80)
    tf = N.NYU_Depth_V2.get_transform(training=False)
    vals = []
    for j in range(2):
        img, _ = N.transform_chw(tf, [ims[j], nyu_chain.raw_test_depths(1, "nyu:val", 60, 80)[0]])
        vals.append(img.numpy())
    out["val_img"] = np.stack(vals)
    out["val_shape"] = np.asarray([60, 80])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
