#!/usr/bin/env python3
"""Generate tests/golden/pose_eval.npz by running the REFERENCE's own kitti_eval/pose_evaluation_utils.py (build container only) on the
tree tests/pose_eval_tree.py writes.

    python tests/golden/make_pose_eval_goldens.py        # DISPNET_REFERENCE=<path> overrides the default reference location

The module is imported as it is; what this container lacks is shimmed, in the style of make_kitti_prep_goldens.py:
  * `path.Path` (path.py is not installed): a str subclass with the methods the module calls (/, dirs(pattern), files(pattern), name);
    both listings are sorted;
  * scipy.misc.imread (removed from SciPy) through PIL: np.asarray(Image.open(f));
  * tqdm, where it is not installed: the identity;
  * np.stack of a generator (this numpy refuses one): the generator is made a list for the duration of the run.
The framework runs once per sequence and snippet length (3 and 5), so that the order of the reference's set of sequences does not
matter.  The file stores, per (sequence, L): the snippet indices, the compensated poses of every snippet and the image paths relative to
the root.  Only numbers and names are stored; nothing of the reference's source is copied.
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

import pose_eval_tree  # noqa: E402

OUT = HERE / "pose_eval.npz"


class Path(str):
    def __truediv__(self, other):
        return Path(os.path.join(self, other))

    @property
    def name(self):
        return Path(os.path.basename(self))

    def dirs(self, pattern="*"):
        return [self / n for n in sorted(os.listdir(self)) if os.path.isdir(os.path.join(self, n)) and fnmatch.fnmatch(n, pattern)]

    def files(self, pattern="*"):
        return [self / n for n in sorted(os.listdir(self)) if os.path.isfile(os.path.join(self, n)) and fnmatch.fnmatch(n, pattern)]


def _install_shims():
    from PIL import Image
    import scipy
    mod = types.ModuleType("path")
    mod.Path = Path
    misc = types.ModuleType("scipy.misc")
    misc.imread = lambda f: np.asarray(Image.open(str(f)))
    scipy.misc = misc
    sys.modules.update({"path": mod, "scipy.misc": misc})
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = t


def _load_reference():
    _install_shims()
    spec = importlib.util.spec_from_file_location("ref_pose_evaluation_utils", REF / "kitti_eval" / "pose_evaluation_utils.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ref = _load_reference()
    stack = np.stack
    np.stack = lambda arrays, *a, **k: stack(list(arrays), *a, **k)
    out = {}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            root = pose_eval_tree.write_odometry(os.path.join(tmp, "odometry"))
            for name, n in pose_eval_tree.GOLDEN_SEQUENCES:
                for L in pose_eval_tree.GOLDEN_LENGTHS:
                    fw = ref.test_framework_KITTI(root, [name], seq_length=L)
                    assert len(fw.img_files) == 1 and len(fw.img_files[0]) == n
                    key = "%s:L%d" % (name, L)
                    samples = list(fw)
                    out[key + ":indices"] = np.asarray(fw.sample_indices[0], dtype=np.int64).reshape(-1, L)
                    out[key + ":poses"] = np.array([s["poses"] for s in samples], dtype=np.float64).reshape(-1, L, 3, 4)
                    out[key + ":files"] = np.array([os.path.relpath(str(f), root) for f in fw.img_files[0]])
                    assert all(len(s["imgs"]) == L and s["imgs"][0].shape == pose_eval_tree.GOLDEN_SIZE + (3,) for s in samples)
    finally:
        np.stack = stack
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays,", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
