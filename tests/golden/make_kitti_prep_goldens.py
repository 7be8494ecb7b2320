#!/usr/bin/env python3
"""Generate tests/golden/kitti_prep.npz by running the REFERENCE's own data/kitti_raw_loader.py (build container only) on the tree
tests/kitti_raw_tree.py writes.

    python tests/golden/make_kitti_prep_goldens.py        # DISPNET_REFERENCE=<path> overrides the default reference location

The loader is imported as it is; what this container lacks is shimmed:
  * `path.Path` (path.py is not installed): a str subclass with the handful of methods the loader calls (/, +, realpath, dirname, dirs,
    files, isfile, name, parent); dirs() and files() are sorted;
  * scipy.misc.imread / imresize (removed from SciPy) through PIL: imread = np.asarray(Image.open(f)); imresize of a uint8 array =
    Image.resize(BILINEAR) with no stretch, which is what bytescale did for uint8 input;
  * np.int (removed from numpy) = int.
The loader runs at 16 x 48 with depth-size ratio 1 and 2, once with the speed rule and once with a static-frames file.  The file stores,
per run and scene: the selected frame ids, P_rect, the intrinsics, the poses and the depth maps as non-zero (y, x) plus fp32 values.
Only numbers are stored; nothing of the reference's source is copied.
"""
import fnmatch
import importlib.util
import os
import pathlib
import sys
import tempfile
import types

import numpy as np

REF = pathlib.Path(os.environ.get("DISPNET_REFERENCE", "/root/reference"))
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import kitti_raw_tree  # noqa: E402

OUT = HERE / "kitti_prep.npz"
HEIGHT, WIDTH = 16, 48


class Path(str):
    def __truediv__(self, other):
        return Path(os.path.join(self, other))

    def __add__(self, other):
        return Path(str.__add__(self, other))

    def realpath(self):
        return Path(os.path.realpath(self))

    def dirname(self):
        return Path(os.path.dirname(self))

    @property
    def parent(self):
        return Path(os.path.dirname(self))

    @property
    def name(self):
        return Path(os.path.basename(self))

    def isfile(self):
        return os.path.isfile(self)

    def dirs(self):
        return [self / n for n in sorted(os.listdir(self)) if os.path.isdir(os.path.join(self, n))]

    def files(self, pattern="*"):
        return [self / n for n in sorted(os.listdir(self)) if os.path.isfile(os.path.join(self, n)) and fnmatch.fnmatch(n, pattern)]


def _install_shims():
    from PIL import Image
    import scipy
    mod = types.ModuleType("path")
    mod.Path = Path
    misc = types.ModuleType("scipy.misc")
    misc.imread = lambda f: np.asarray(Image.open(str(f)))

    def imresize(arr, size):
        assert arr.dtype == np.uint8
        return np.asarray(Image.fromarray(arr).resize((int(size[1]), int(size[0])), resample=Image.BILINEAR))

    misc.imresize = imresize
    scipy.misc = misc
    sys.modules.update({"path": mod, "scipy.misc": misc})
    if not hasattr(np, "int"):
        np.int = int


def _load_reference():
    _install_shims()
    spec = importlib.util.spec_from_file_location("ref_kitti_raw_loader", REF / "data" / "kitti_raw_loader.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ref = _load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tree = kitti_raw_tree.write_tree(os.path.join(tmp, "raw"))
        static = kitti_raw_tree.write_static_frames(os.path.join(tmp, "static.txt"))
        for date in ("2011_09_29", "2011_09_30", "2011_10_03"):
            os.makedirs(os.path.join(tree, date), exist_ok=True)      # the loader lists all five dates; these three stay empty
        for mode, static_file in (("speed", None), ("static", static)):
            for ratio in (1, 2):
                loader = ref.KittiRawLoader(tree, static_frames_file=static_file, img_height=HEIGHT, img_width=WIDTH, get_depth=True,
                                            get_pose=True, depth_size_ratio=ratio)
                run = "%s:r%d" % (mode, ratio)
                names = []
                for drive in loader.scenes:
                    for scene in loader.collect_scenes(drive):
                        key = run + ":" + scene["rel_path"]
                        names.append(scene["rel_path"])
                        samples = list(loader.get_scene_imgs(scene))
                        out[key + ":ids"] = np.array([int(s["id"]) for s in samples], dtype=np.int64)
                        out[key + ":P_rect"] = np.asarray(scene["P_rect"], dtype=np.float64)
                        out[key + ":intrinsics"] = np.asarray(scene["intrinsics"], dtype=np.float64)
                        out[key + ":poses"] = np.array([s["pose"] for s in samples], dtype=np.float64).reshape(-1, 12)
                        for s in samples:
                            d = s["depth"]
                            assert d.dtype == np.float32 and d.shape == (HEIGHT // ratio, WIDTH // ratio)
                            yy, xx = np.nonzero(d)
                            out["%s:depth:%s:yx" % (key, s["id"])] = np.stack([yy, xx], 1).astype(np.uint8)
                            out["%s:depth:%s:val" % (key, s["id"])] = d[yy, xx]
                out[run + ":scenes"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays,", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
