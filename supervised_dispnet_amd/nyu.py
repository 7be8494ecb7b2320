"""NYU Depth v2 (reference datasets/nyu_depth_v2.py) with its augmentation chain on the GPU.

On disk (reference data/nyudepth_preparation):
  * training: DATA/nyu_depth_v2_other_resolution/npy/*.npy, sorted by name, each a (5, H0, W0) float32 array -- RGB in 0..255,
    depth in metres, a 0/1 mask;
  * validation: DATA/nyu_depth_v2_other_resolution/labeled/npy/{images,depths}.npy, (N,3,480,640) and (N,1,480,640) float32.

The reference augments each training sample on a DataLoader worker in numpy (flip, cubic-spline rotation, crop, bilinear zoom,
colour gain, Normalize).  Here the host only draws the parameters -- `draw_params`, the reference's draw order and count -- and
gathers the raw arrays into pinned buffers; dn_nyu_prefilter / dn_nyu_train_resample (csrc/dn_nyu.hip) compute the batch on the
device.  Validation images go through dn_nyu_val_resize (scipy.ndimage.zoom(order=1) to 320x448 + Normalize).  Normalisation is
always the ImageNet mean / std the reference's NYU loader hard-codes, whatever --imagenet-normalization says.

Reproducibility: sample `index` of epoch `epoch` draws from its own np.random.RandomState(sample_seed(seed, epoch, index)), so its
augmentation depends on neither the number of ranks nor thread timing.
"""
import concurrent.futures
import os
import queue
import threading

import numpy as np
import torch

from . import engine

NYUD_MEAN = (0.485, 0.456, 0.406)
NYUD_STD = (0.229, 0.224, 0.225)
TRAIN_SIZE = (256, 352)          # get_transform(training=True, size=(256, 352)): the crop every training sample ends at
VAL_SIZE = (320, 448)            # BilinearResize(320/480, 448/640)
MINMAX_CHUNKS = 16               # DN_NYU_MINMAX_CHUNKS
MAX_READERS = 16

_C = __import__("ctypes")
_MEAN_H = (_C.c_float * 3)(*NYUD_MEAN)
_STD_H = (_C.c_float * 3)(*NYUD_STD)


def train_dir(root):
    return os.path.join(root, "nyu_depth_v2_other_resolution", "npy")


def test_dir(root):
    return os.path.join(root, "nyu_depth_v2_other_resolution", "labeled", "npy")


def sample_seed(seed, epoch, index):
    """Seed of sample `index`'s RandomState in `epoch`: ((seed * 1000003 + epoch) * 1000003 + index) mod 2**32."""
    return ((int(seed) * 1000003 + int(epoch)) * 1000003 + int(index)) % (1 << 32)


def check_size(H0, W0, size=TRAIN_SIZE):
    """The reference's RandomCropNumpy is right only when both sides exceed the crop or both equal it (its two mixed branches put the
    draw on the wrong axis and return a mis-shaped crop): refuse the rest."""
    th, tw = size
    if (H0, W0) == (th, tw) or (H0 > th and W0 > tw):
        return
    raise ValueError("NYU training samples of {}x{} cannot be cropped to {}x{}: the reference's crop needs both sides larger than the "
                     "crop or both equal to it".format(H0, W0, th, tw))


def draw_params(rs, H0, W0, size=TRAIN_SIZE):
    """One sample's draws with the reference's order and count (nyu_depth_v2.py:76-110): flip (uniform() > 0.5), angle U(-5, 5),
    crop row then column (randint, high end exclusive; no draw at exactly `size`), zoom U(1.0, 1.5), colour gain U(0.8, 1.2).
    Returns (flip, angle, r0, c0, s, mult)."""
    check_size(H0, W0, size)
    th, tw = size
    flip = rs.uniform() > 0.5
    angle = rs.uniform(-5, 5)
    if (H0, W0) == (th, tw):
        r0 = c0 = 0
    else:
        r0 = rs.randint(0, H0 - th)
        c0 = rs.randint(0, W0 - tw)
    s = rs.uniform(1.0, 1.5)
    mult = rs.uniform(0.8, 1.2)
    return (bool(flip), float(angle), int(r0), int(c0), float(s), float(mult))


def params_array(draws):
    """[(flip, angle, r0, c0, s, mult), ...] -> float64 [B, 8], the layout dn_nyu_train_resample reads."""
    p = np.zeros((len(draws), 8), dtype=np.float64)
    for j, d in enumerate(draws):
        if not 1.0 <= d[4] <= 1.5 + 1e-12:
            raise ValueError("zoom %r outside [1, 1.5]" % (d[4],))
        p[j, :6] = d
    return p


def augment_batch(raw, params, size=TRAIN_SIZE, workspace=None):
    """raw: device [B,5,H0,W0] float32; params: device [B,8] float64 (params_array) -> (img [B,3,th,tw], depth [B,th,tw]) on the
    current stream.  `workspace` = (coef, minmax) device buffers to reuse, else allocated here."""
    engine.require_cuda(raw, "augment_batch raw")
    if raw.dtype != torch.float32 or raw.dim() != 4 or raw.shape[1] != 5 or not raw.is_contiguous():
        raise ValueError("raw must be a contiguous float32 [B,5,H0,W0] tensor, got %s %s" % (raw.dtype, tuple(raw.shape)))
    if params.dtype != torch.float64 or tuple(params.shape) != (raw.shape[0], 8) or not params.is_contiguous() or params.device != raw.device:
        raise ValueError("params must be a contiguous float64 [B,8] tensor on the raw batch's device")
    B, _, H0, W0 = raw.shape
    th, tw = size
    if th > H0 or tw > W0:
        raise ValueError("crop %dx%d exceeds the sample's %dx%d" % (th, tw, H0, W0))
    if workspace is None:
        workspace = new_workspace(B, H0, W0, raw.device)
    coef, mm = workspace
    img = torch.empty((B, 3, th, tw), dtype=torch.float32, device=raw.device)
    depth = torch.empty((B, th, tw), dtype=torch.float32, device=raw.device)
    st = torch.cuda.current_stream(raw.device).cuda_stream
    engine.hbm_call("dn::nyu_prefilter_cols_kernel", B * H0 * W0 * (20 + 64), "dn_nyu_prefilter", raw.data_ptr(), params.data_ptr(), B, H0, W0, coef.data_ptr(),
                    mm.data_ptr(), st)
    engine.hbm_call("dn::nyu_train_resample_kernel", B * (H0 * W0 * 32 + th * tw * 16), "dn_nyu_train_resample", coef.data_ptr(), mm.data_ptr(),
                    params.data_ptr(), B, H0, W0, th, tw, _MEAN_H, _STD_H, img.data_ptr(), depth.data_ptr(), st)
    return img, depth


def new_workspace(B, H0, W0, device):
    return (torch.empty((B, 4, H0, W0), dtype=torch.float64, device=device),
            torch.empty((B, MINMAX_CHUNKS, 2), dtype=torch.float32, device=device))


def resize_batch(images, size=VAL_SIZE):
    """images: device [B,3,IH,IW] float32 (0..255) -> [B,3,oh,ow] normalised (BilinearResize + ToTensor + Normalize)."""
    engine.require_cuda(images, "resize_batch images")
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 3 or not images.is_contiguous():
        raise ValueError("images must be a contiguous float32 [B,3,H,W] tensor, got %s %s" % (images.dtype, tuple(images.shape)))
    B, _, IH, IW = images.shape
    oh, ow = size
    out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=images.device)
    engine.hbm_call("dn::nyu_val_resize_kernel", B * 3 * (IH * IW + oh * ow) * 4, "dn_nyu_val_resize", images.data_ptr(), B, IH, IW, oh, ow,
                    _MEAN_H, _STD_H, out.data_ptr(), torch.cuda.current_stream(images.device).cuda_stream)
    return out


class NyuTrainSet(object):
    """DATA/nyu_depth_v2_other_resolution/npy/*.npy, sorted by name (nyu_depth_v2.py:42-43)."""

    def __init__(self, root, size=TRAIN_SIZE):
        folder = train_dir(root)
        if not os.path.isdir(folder):
            raise FileNotFoundError("NYU training folder {} not found".format(folder))
        self.file_paths = [os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.endswith(".npy")]
        if not self.file_paths:
            raise ValueError("no .npy sample under {}".format(folder))
        first = np.load(self.file_paths[0], mmap_mode="r")
        if first.dtype != np.float32 or first.ndim != 3 or first.shape[0] != 5:
            raise ValueError("{}: expected a (5, H0, W0) float32 array, got {} {}".format(self.file_paths[0], first.dtype, first.shape))
        self.H0, self.W0 = int(first.shape[1]), int(first.shape[2])
        check_size(self.H0, self.W0, size)
        self.size = size
        self.scenes = [folder]

    def __len__(self):
        return len(self.file_paths)

    def read_into(self, index, out):
        a = np.load(self.file_paths[index], mmap_mode="r")
        if a.shape != (5, self.H0, self.W0) or a.dtype != np.float32:
            raise ValueError("{}: {} {} differs from the first sample's (5, {}, {}) float32".format(
                self.file_paths[index], a.dtype, a.shape, self.H0, self.W0))
        out[...] = a

    def __getitem__(self, index):
        out = np.empty((5, self.H0, self.W0), dtype=np.float32)
        self.read_into(index, out)
        return out


class NyuTestSet(object):
    """DATA/nyu_depth_v2_other_resolution/labeled/npy/{images,depths}.npy, memory-mapped (nyu_depth_v2.py:37-40)."""

    def __init__(self, root):
        folder = test_dir(root)
        self.images = np.load(os.path.join(folder, "images.npy"), mmap_mode="r")
        self.depths = np.load(os.path.join(folder, "depths.npy"), mmap_mode="r")
        n = len(self.images)
        if self.images.ndim != 4 or self.images.shape[1] != 3 or self.images.dtype != np.float32:
            raise ValueError("images.npy: expected (N,3,H,W) float32, got {} {}".format(self.images.dtype, self.images.shape))
        if self.depths.shape != (n, 1) + self.images.shape[2:] or self.depths.dtype != np.float32:
            raise ValueError("depths.npy: expected {} float32, got {} {}".format((n, 1) + self.images.shape[2:], self.depths.dtype, self.depths.shape))
        self.H, self.W = int(self.images.shape[2]), int(self.images.shape[3])
        self.scenes = [folder]

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        return np.asarray(self.images[index]), np.asarray(self.depths[index, 0])


class NyuLoader(object):
    """Iterable over device-resident NYU batches, modelled on shards.ShardLoader.  train=True yields (img [B,3,256,352],
    depth [B,256,352]); train=False yields (img [B,3,320,448], depth [B,480,640]).  Every rank walks the same order and keeps its
    contiguous slice of each global batch (data.RankSampler).  A producer thread reads the samples with up to 16 reader threads into
    pinned staging buffers and copies them on a side stream; the kernels run on the consumer's current stream."""

    def __init__(self, root, batch_size, device, train=True, seed=0, rank=0, world=1, shuffle=None, drop_last=None, prefetch=2,
                 readers=MAX_READERS, dataset=None):
        from .data import RankSampler
        self.train = bool(train)
        self.set = dataset if dataset is not None else (NyuTrainSet(root) if self.train else NyuTestSet(root))
        self.device = torch.device(device)
        engine.require_cuda(torch.empty(0, device=self.device), "NyuLoader device")
        self.B = int(batch_size)
        shuffle = self.train if shuffle is None else shuffle
        drop_last = self.train if drop_last is None else drop_last
        self.sampler = RankSampler(len(self.set), self.B * world, rank, world, shuffle, seed=seed, drop_last=drop_last)
        self.seed, self.epoch = int(seed or 0), 0
        self.prefetch = max(1, int(prefetch))
        self.readers = max(1, min(MAX_READERS, int(readers), self.B))
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._ring, self._slot = [], 0
        self._ws = None

    def set_epoch(self, epoch):
        self.sampler.set_epoch(epoch)
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.sampler)

    def draws(self, idxs, epoch=None):
        """The draws of dataset samples `idxs` in `epoch` (default: the current one)."""
        e = self.epoch if epoch is None else epoch
        return [draw_params(np.random.RandomState(sample_seed(self.seed, e, i)), self.set.H0, self.set.W0) for i in idxs]

    def _staging(self):
        n = self.prefetch + 2
        if not self._ring:
            for _ in range(n):
                if self.train:
                    slot = {"raw": torch.empty((self.B, 5, self.set.H0, self.set.W0), dtype=torch.float32).pin_memory(),
                            "par": torch.empty((self.B, 8), dtype=torch.float64).pin_memory()}
                else:
                    slot = {"img": torch.empty((self.B, 3, self.set.H, self.set.W), dtype=torch.float32).pin_memory(),
                            "dep": torch.empty((self.B, self.set.H, self.set.W), dtype=torch.float32).pin_memory()}
                slot["ev"] = None
                self._ring.append(slot)
        slot = self._ring[self._slot]
        self._slot = (self._slot + 1) % n
        if slot["ev"] is not None:
            slot["ev"].synchronize()             # the copy that last read this slot is done
        return slot

    def _stage(self, idxs, pool):
        b = len(idxs)
        slot = self._staging()
        with torch.cuda.stream(self.copy_stream):
            if self.train:
                raw, par = slot["raw"][:b], slot["par"][:b]
                rawn = raw.numpy()
                list(pool.map(lambda jk: self.set.read_into(jk[1], rawn[jk[0]]), enumerate(idxs)))
                par.numpy()[:] = params_array(self.draws(idxs))
                out = (torch.empty(raw.shape, dtype=torch.float32, device=self.device),
                       torch.empty(par.shape, dtype=torch.float64, device=self.device))
                out[0].copy_(raw, non_blocking=True)
                out[1].copy_(par, non_blocking=True)
            else:
                img, dep = slot["img"][:b], slot["dep"][:b]
                imgn, depn = img.numpy(), dep.numpy()

                def read(jk):
                    imgn[jk[0]] = self.set.images[jk[1]]
                    depn[jk[0]] = self.set.depths[jk[1], 0]

                list(pool.map(read, enumerate(idxs)))
                out = (torch.empty(img.shape, dtype=torch.float32, device=self.device),
                       torch.empty(dep.shape, dtype=torch.float32, device=self.device))
                out[0].copy_(img, non_blocking=True)
                out[1].copy_(dep, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        slot["ev"] = ev
        return out, ev

    def _finish(self, staged):
        (a, b), ev = staged
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        a.record_stream(cur)
        b.record_stream(cur)
        if not self.train:
            return resize_batch(a), b
        B, _, H0, W0 = a.shape
        if self._ws is None or self._ws[0].shape[0] < B:
            self._ws = new_workspace(B, H0, W0, self.device)
        return augment_batch(a, b, workspace=(self._ws[0][:B], self._ws[1][:B]))

    def __iter__(self):
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def producer():
            try:
                torch.cuda.set_device(self.device)
                with concurrent.futures.ThreadPoolExecutor(max_workers=self.readers) as pool:
                    for idxs in self.sampler:
                        if stop.is_set():
                            return
                        q.put(self._stage(idxs, pool))
                q.put(None)
            except BaseException as e:      # noqa: BLE001 -- surfaced on the consumer side
                q.put(e)

        t = threading.Thread(target=producer, daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield self._finish(item)
        finally:
            stop.set()
            while t.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                t.join(timeout=0.05)
