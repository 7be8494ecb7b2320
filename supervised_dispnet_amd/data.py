"""Host-side sample sources for train.py / test_disp.py.

Only what the training hot path needs to be driven from the reference's on-disk layouts (the data pipeline itself is out of
scope): the scene-folder format of datasets/sequence_folders.py:14-76 and
datasets/validation_folders.py:28-60 (JPEG frames + per-frame .npy depth + cam.txt), the reference's transform chain
(custom_transforms.py: RandomHorizontalFlip 56-72, ArrayToTensor 40-53 with its /255, Normalize 25-37), and a synthetic
source with the statistics of SURVEY.md section 8d for boxes without a dataset.  JPEG decode is PIL (imageio is absent).
"""
import os
import random

import numpy as np
import torch
import torch.utils.data as data


def load_as_float(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.float32)


def normalization(imagenet=False, monodepth2=False):
    """(mean, std) of train.py:121-132 / test_disp.py:203-211."""
    if imagenet:
        return ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0]) if monodepth2 else ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    return [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]


SCALE_CROP_MAX = 1.15     # custom_transforms.py:81: up to 15 % per axis


def draw_scale_crop(rng, H, W):
    """The draws of custom_transforms.RandomScaleCrop (:81-82, :104-105) from `rng` (numpy.random or a RandomState), in its order:
    -> (sx, sy, sh, sw, oy, ox).  The scaled size is the fp64 product, truncated."""
    sx, sy = rng.uniform(1, SCALE_CROP_MAX, 2)
    sh, sw = int(H * sy), int(W * sx)
    oy = rng.randint(sh - H + 1)
    ox = rng.randint(sw - W + 1)
    return float(sx), float(sy), sh, sw, int(oy), int(ox)


def scale_crop_intrinsics(intrinsics, sx, sy, oy, ox):
    """Rows 0 / 1 times sx / sy, then the principal point minus the crop offset: every step in fp64, rounded to fp32 once."""
    k = np.array(intrinsics, dtype=np.float32)
    k[0] = (k[0].astype(np.float64) * sx).astype(np.float32)
    k[1] = (k[1].astype(np.float64) * sy).astype(np.float32)
    k[0, 2] = np.float32(np.float64(k[0, 2]) - ox)
    k[1, 2] = np.float32(np.float64(k[1, 2]) - oy)
    return k


def bytescale(a):
    """scipy.misc.bytescale of a float32 array by its own min / max: uint8(clip(fp32((a - min) * fp32(255 / (max - min))) + 0.5, 0, 255)),
    scale 1 for a constant array (DESIGN.md sections 11 and 14)."""
    a = np.asarray(a, dtype=np.float32)
    cmin, cmax = float(a.min()), float(a.max())
    scale = np.float32(255.0 / (cmax - cmin) if cmax > cmin else 1.0)
    t = (a - np.float32(cmin)) * scale + np.float32(0.5)
    return np.clip(t, 0, 255).astype(np.uint8)


def imresize_crop(a, sh, sw, oy, ox):
    """scipy.misc.imresize(a, (sh, sw))[oy:oy + H, ox:ox + W] of a float32 [H, W, 3] frame or [H, W] map -> uint8: byte-scale, then
    Pillow's 8-bit bilinear resize (a no-op for an axis that keeps its size), then the crop."""
    from PIL import Image
    H, W = a.shape[:2]
    im = Image.fromarray(bytescale(a)).resize((sw, sh), Image.BILINEAR)
    return np.array(im)[oy:oy + H, ox:ox + W]


def draw_colour_jitter(rng, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, prob=0.5):
    """monodepth2's colour jitter draw for one sample (all its frames share it) from `rng` (numpy.random or a RandomState): always the
    same seven calls in the same order, whether or not the sample is jittered, so a sample's draw never moves the next one's.
    -> None, or (order, b, c, s, shift): the order of the four operations (0 brightness, 1 contrast, 2 saturation, 3 hue), the three
    factors and the hue shift in Pillow's 8-bit hue units, np.uint8(h * 255) as torchvision forms it (truncated, then mod 256)."""
    u = rng.random_sample()
    order = rng.permutation(4)
    b = rng.uniform(1 - brightness, 1 + brightness)
    c = rng.uniform(1 - contrast, 1 + contrast)
    s = rng.uniform(1 - saturation, 1 + saturation)
    h = rng.uniform(-hue, hue)
    if not u > prob:
        return None
    return tuple(int(o) for o in order), float(b), float(c), float(s), int(h * 255) % 256


def colour_jitter_u8(frame, params):
    """The jitter of one uint8 [H, W, 3] frame (or a float array holding such integers) with Pillow itself, operation by operation as
    torchvision's ColorJitter applies them: ImageEnhance.Brightness / Contrast / Color, and the HSV round trip with the hue channel
    shifted mod 256 (taken also when the shift is 0).  The host statement of dn_colour_jitter_*; the JPEG loader runs it."""
    a = np.ascontiguousarray(np.asarray(frame).astype(np.uint8))
    if params is None:
        return a
    from PIL import Image, ImageEnhance
    order, b, c, s, shift = params
    im = Image.fromarray(a)
    for op in order:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(b)
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(c)
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(s)
        else:
            h, sat, v = im.convert("HSV").split()
            nh = ((np.asarray(h, dtype=np.int32) + int(shift)) % 256).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(nh), sat, v)).convert("RGB")
    return np.asarray(im, dtype=np.uint8)


class Transform(object):
    """[colour jitter (train only)] -> flip (train only) -> [scale and crop (train only)] -> CHW float /255 -> normalise, applied
    coherently to images, depth and intrinsics.  `scale_crop` is the reference's RandomScaleCrop (custom_transforms.py:73-113) in its
    Compose position, drawn from the global numpy.random as the reference's workers do; it is the host statement of what
    dn_scale_crop_u8 / _depth compute.  `color_aug` is monodepth2's colour jitter (draw_colour_jitter / colour_jitter_u8, DESIGN.md
    section 19) on the decoded frames, one draw per sample from the global numpy.random in front of the scale-crop draws; with
    `keep_plain` the returned list holds the n augmented tensors followed by the n plain ones (same flip, same crop)."""

    def __init__(self, mean, std, flip, scale_crop=False, color_aug=False, keep_plain=False):
        self.mean = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
        self.flip = flip
        self.scale_crop = scale_crop
        self.color_aug = color_aug
        self.keep_plain = bool(color_aug and keep_plain)

    def __call__(self, images, gt_depth, intrinsics):
        flip = bool(self.flip and random.random() < 0.5)
        jitter = draw_colour_jitter(np.random) if self.color_aug else None
        crop = draw_scale_crop(np.random, *images[0].shape[:2]) if self.scale_crop else None
        if not self.color_aug:
            return self.apply(images, gt_depth, intrinsics, flip, crop)
        frames = [colour_jitter_u8(im, jitter).astype(np.float32) for im in images]
        # one pass for both halves: every frame takes the chain on its own, the depth and the intrinsics are done once
        return self.apply(frames + list(images) if self.keep_plain else frames, gt_depth, intrinsics, flip, crop)

    def apply(self, images, gt_depth, intrinsics, flip, crop=None):
        """The chain behind the colour jitter for given draws: flip (bool) and crop = (sx, sy, sh, sw, oy, ox) or None."""
        if flip:
            images = [np.ascontiguousarray(np.fliplr(im)) for im in images]
            gt_depth = np.ascontiguousarray(np.fliplr(gt_depth))
            if intrinsics is not None:
                intrinsics = np.copy(intrinsics)
                intrinsics[0, 2] = images[0].shape[1] - intrinsics[0, 2]
        if crop is not None:
            sx, sy, sh, sw, oy, ox = crop
            images = [imresize_crop(im, sh, sw, oy, ox) for im in images]
            gmax = float(np.max(np.asarray(gt_depth, dtype=np.float32)))                      # the maximum only (:92-93)
            gt_depth = (imresize_crop(gt_depth, sh, sw, oy, ox).astype(np.float64) / 255.0 * gmax).astype(np.float32)
            if intrinsics is not None:
                intrinsics = scale_crop_intrinsics(intrinsics, sx, sy, oy, ox)
        tensors = [(torch.from_numpy(np.transpose(im, (2, 0, 1))).float() / 255 - self.mean) / self.std for im in images]
        return tensors, torch.from_numpy(np.ascontiguousarray(gt_depth)).float(), intrinsics


def _scenes(root, list_name):
    with open(os.path.join(root, list_name)) as f:
        return [os.path.join(root, line.strip()) for line in f if line.strip()]


def _files(folder, ext):
    return sorted(os.path.join(folder, n) for n in os.listdir(folder) if n.endswith(ext))


class SequenceFolder(data.Dataset):
    """root/scene/{0000000.jpg, 0000000.npy, ..., cam.txt}; train.txt / val.txt list the scenes.
    Yields (tgt_img, gt_depth) -- or (tgt_img, ref_imgs, intrinsics, intrinsics_inv, gt_depth) with `with_refs`, the
    5-tuple the reference's --unsupervised branch expects but its loader no longer returns.  A transform with
    `keep_plain` (Transform(color_aug=True, keep_plain=True)) adds a sixth entry, the unjittered frames [tgt, refs...]; every other
    sample keeps its layout."""

    def __init__(self, root, seed=None, train=True, sequence_length=3, transform=None, percentage=1, with_refs=False):
        np.random.seed(seed)
        random.seed(seed)
        self.scenes = _scenes(root, "train.txt" if train else "val.txt")
        self.transform = transform
        self.with_refs = with_refs
        demi = (sequence_length - 1) // 2
        shifts = [s for s in range(-demi, demi + 1) if s != 0]
        samples = []
        for scene in self.scenes:
            intr = np.genfromtxt(os.path.join(scene, "cam.txt")).astype(np.float32).reshape(3, 3)
            imgs, depth = _files(scene, ".jpg"), _files(scene, ".npy")
            if len(imgs) < sequence_length:
                continue
            for i in range(demi, len(imgs) - demi):
                samples.append({"intrinsics": intr, "tgt": imgs[i], "ref_imgs": [imgs[i + s] for s in shifts], "gt_depth": depth[i]})
        random.shuffle(samples)
        self.samples = samples[:int(percentage * len(samples))]

    def __getitem__(self, index):
        s = self.samples[index]
        imgs = [load_as_float(s["tgt"])] + ([load_as_float(r) for r in s["ref_imgs"]] if self.with_refs else [])
        gt = np.load(s["gt_depth"]).astype(np.float32)
        intr = np.copy(s["intrinsics"])
        n = len(imgs)
        if self.transform is not None:
            imgs, gt, intr = self.transform(imgs, gt, intr)
        if self.with_refs:
            if getattr(self.transform, "keep_plain", False):     # a sixth entry, the plain frames in the order [tgt, refs...]
                return imgs[0], imgs[1:n], intr, np.linalg.inv(intr), gt, imgs[n:]
            return imgs[0], imgs[1:], intr, np.linalg.inv(intr), gt
        return imgs[0], gt

    def __len__(self):
        return len(self.samples)


class ValidationSet(data.Dataset):
    """root/scene/{0000000.jpg, 0000000.npy, ...} listed by val.txt -> (img, depth)."""

    def __init__(self, root, transform=None):
        self.scenes = _scenes(root, "val.txt")
        self.imgs, self.depth = [], []
        for scene in self.scenes:
            for img in _files(scene, ".jpg"):
                d = img[:-4] + ".npy"
                if not os.path.isfile(d):
                    raise FileNotFoundError("depth file {} not found".format(d))
                self.imgs.append(img)
                self.depth.append(d)
        self.transform = transform

    def __getitem__(self, index):
        img = load_as_float(self.imgs[index])
        depth = np.load(self.depth[index]).astype(np.float32)
        if self.transform is not None:
            t, _, _ = self.transform([img], depth, None)
            img = t[0]
        return img, torch.from_numpy(depth)

    def __len__(self):
        return len(self.imgs)


class SyntheticDepthSet(data.Dataset):
    """SURVEY.md section 8d inputs: image U(0,1) normalised with mean = std = 0.5; ground truth U(1, max) where a
    Bernoulli(density) mask is set, 0 elsewhere.  Deterministic per index."""

    def __init__(self, length, height=128, width=416, density=0.05, max_depth=80.0, seed=0, sequence_length=3, with_refs=False):
        self.length, self.h, self.w = int(length), height, width
        self.density, self.max_depth, self.seed = density, max_depth, seed
        self.nref = sequence_length - 1
        self.with_refs = with_refs
        self.scenes = ["synthetic"]

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed * 1000003 + index)
        img = (torch.rand(3, self.h, self.w, generator=g) - 0.5) / 0.5
        depth = torch.rand(self.h, self.w, generator=g) * (self.max_depth - 1.0) + 1.0
        gt = depth * (torch.rand(self.h, self.w, generator=g) < self.density).float()
        if not self.with_refs:
            return img, gt
        refs = [(img + 0.05 * torch.randn(3, self.h, self.w, generator=g)).clamp(-1, 1) for _ in range(self.nref)]
        intr = np.array([[241.67, 0, 204.17], [0, 246.28, 59.0], [0, 0, 1]], dtype=np.float32)
        return img, refs, intr, np.linalg.inv(intr), gt

    def __len__(self):
        return self.length


class RankSampler(data.Sampler):
    """Every rank draws the SAME shuffled global order and keeps its contiguous slice of each global batch -- the split
    nn.DataParallel.scatter makes of the reference's batch (train.py:316), one process per GPU instead of one per node.
    With drop_last=False (validation) the last, partial global batch is split into ceil(m / world)-sized contiguous slices
    (again what scatter does); a rank whose slice is empty simply has one batch fewer -- the validation loops carry no
    collective per batch, the (sum, count) all-reduce at their end handles unequal counts."""

    def __init__(self, n, global_batch, rank, world, shuffle, seed=0, drop_last=True):
        if global_batch % world != 0:
            raise ValueError("batch size %d does not divide over %d ranks" % (global_batch, world))
        self.n, self.gb, self.rank, self.world, self.shuffle, self.seed = n, global_batch, rank, world, shuffle, seed
        self.epoch = 0
        self.nbatches = n // global_batch if drop_last else (n + global_batch - 1) // global_batch

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _slice(self, m):
        """[lo, hi) of this rank inside a global batch of m <= gb samples."""
        per = self.gb // self.world if m == self.gb else (m + self.world - 1) // self.world
        return min(self.rank * per, m), min((self.rank + 1) * per, m)

    def __iter__(self):
        order = list(range(self.n))
        if self.shuffle:
            random.Random(self.seed + self.epoch).shuffle(order)
        for b in range(self.nbatches):
            chunk = order[b * self.gb:(b + 1) * self.gb]
            lo, hi = self._slice(len(chunk))
            if hi > lo:
                yield chunk[lo:hi]

    def __len__(self):
        full = self.n // self.gb
        tail = self.n - full * self.gb
        if self.nbatches == full or tail == 0:
            return self.nbatches
        lo, hi = self._slice(tail)
        return full + (1 if hi > lo else 0)
