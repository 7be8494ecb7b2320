"""run_inference.py of the reference (pictures in, disparity and depth images out) with the image arithmetic around the network on
the device (csrc/dn_image.hip).

Per batch the host reads the frames (PIL) and uploads them as they are; the device byte-scales and resizes them like
scipy.misc.imresize (dn_imresize_u8, bit for bit Pillow's bilinear resize), normalises, runs ONE eval-mode forward at batch B, and
colours the outputs: the Garg-crop rectangle of the disparity through 'bone' (dn_colorize_u8) and its contrast-4 enhancement
(dn_contrast_u8), and 1 / disparity with max_value 10 through 'rainbow'.  uint8 images come back and PIL writes them.

--host-chain is the reference's own per-image loop in numpy / PIL -- the same forward, the same files; it is the yardstick and the
place where the semantics are written down in Python (host_preprocess, host_images).

The colour tables are OpenCV's (utils.colour_table); without cv2 both chains take tensor2array's grey branch, as the reference does.
"""
import argparse
import ctypes
import datetime
import functools
import os

import numpy as np
import torch

from . import _lib, kitti_eval as KE
from .evaluation import prefetched

MAX_READERS = 16
IMAGE_CHUNKS = 64          # DN_IMAGE_CHUNKS
MAX_TAPS = 32              # DN_IMRESIZE_MAX_TAPS
PRECISION_BITS = 22        # Pillow: 32 - 8 - 2
CONTRAST = 4.0             # run_inference.py:177
DEPTH_MAX = 10             # run_inference.py:182


# ------------------------------------------------------------------------------------------------ resize coefficients (host, fp64)
@functools.lru_cache(maxsize=None)
def resize_coefficients(n, O):
    """Pillow's bilinear coefficients (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) of one axis, n inputs ->
    O outputs: (first int32 [O], count int32 [O], k int32 [O, T]), T = count.max(); output o is
    clip8((2^21 + sum_j k[o, j] * in[first[o] + j]) >> 22).  All in double, the weights summed in tap order as the C loop does."""
    scale = n / O
    fs = max(scale, 1.0)
    support, ss = 1.0 * fs, 1.0 / fs
    center = (np.arange(O, dtype=np.float64) + 0.5) * scale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)
    last = np.minimum((center + support + 0.5).astype(np.int64), n)
    count = last - first
    T = int(count.max())
    x = np.arange(T, dtype=np.float64)[None, :]
    wgt = np.maximum(0.0, 1.0 - np.abs((x + first[:, None] - center[:, None] + 0.5) * ss))
    wgt[np.arange(T)[None, :] >= count[:, None]] = 0.0
    total = np.zeros(O)
    for j in range(T):
        total = total + wgt[:, j]
    wgt = wgt / total[:, None]
    k = (wgt * (1 << PRECISION_BITS) + 0.5).astype(np.int64)
    return first.astype(np.int32), count.astype(np.int32), k.astype(np.int32)


def table_rows(n, O):
    """The int32 [O, 2 + T] table dn_imresize_u8 reads for one axis: {first, count, k[T]} per output index."""
    first, count, k = resize_coefficients(n, O)
    return np.ascontiguousarray(np.concatenate([first[:, None], count[:, None], k], axis=1), dtype=np.int32)


SCALE_CROP_TAPS = 3       # DN_SCALE_CROP_TAPS


@functools.lru_cache(maxsize=None)
def _scale_crop_axis(n, O):
    """The int32 [O, 4] rows {first, k0, k1, k2} of one upscaled axis for dn_scale_crop_u8 / _depth (n inputs -> O >= n outputs), and
    the largest tap count.  O == n is the skipped pass, written as the identity {index, 1 << 22, 0, 0}."""
    if O < n:
        raise ValueError("scale-and-crop never shrinks an axis: {} -> {}".format(n, O))
    rows = np.zeros((O, 1 + SCALE_CROP_TAPS), dtype=np.int32)
    if O == n:
        rows[:, 0] = np.arange(n)
        rows[:, 1] = 1 << PRECISION_BITS
        rows.setflags(write=False)
        return rows, 1
    first, count, k = resize_coefficients(n, O)
    taps = int(count.max())
    if taps > SCALE_CROP_TAPS:                       # cannot happen: upscaling has support 1
        raise ValueError("{} taps per output for the axis {} -> {}; the table rows hold {}".format(taps, n, O, SCALE_CROP_TAPS))
    rows[:, 0] = first
    rows[:, 1:1 + k.shape[1]] = k
    rows.setflags(write=False)
    return rows, taps


def scale_crop_rows(n, O, o0):
    """-> (int32 [n, 4], taps): the rows of outputs [o0, o0 + n) of the axis n -> O, i.e. of the crop window that starts at o0."""
    rows, taps = _scale_crop_axis(int(n), int(O))
    if not 0 <= o0 <= O - n:
        raise ValueError("crop offset {} outside [0, {}]".format(o0, O - n))
    return rows[o0:o0 + n], taps


def scale_crop_table(H, W, draws, out=None):
    """The per-sample table int32 [B, W + H, 4] of the draws [(sh, sw, oy, ox)]: the W crop columns, then the H crop rows.
    -> (table, largest tap count).  `out`: a buffer to fill (the loader's pinned staging)."""
    B = len(draws)
    table = np.empty((B, W + H, 4), dtype=np.int32) if out is None else out
    taps = 1
    for b, (sh, sw, oy, ox) in enumerate(draws):
        table[b, :W], tx = scale_crop_rows(W, sw, ox)
        table[b, W:], ty = scale_crop_rows(H, sh, oy)
        taps = max(taps, tx, ty)
    return table, taps


def check_frame(frame, name):
    a = np.asarray(frame)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("{}: a frame of shape {} and type {} -- H x W x 3 uint8 (RGB) frames only; grey and RGBA inputs fail in the "
                         "reference too".format(name, a.shape, a.dtype))
    return a


def garg_rectangle(h, w):
    """run_inference.py:158-160 -> (r0, r1, c0, c1) at network resolution."""
    return tuple(int(v) for v in (0.40810811 * h, 0.99189189 * h, 0.03594771 * w, 0.96405229 * w))


# ------------------------------------------------------------------------------------------------ the device side
class ImageOps(object):
    """dn_imresize_u8 / dn_colorize_u8 / dn_contrast_u8 on torch tensors of one device.  Workspaces and the pool of coefficient tables
    grow to what has been seen and are reused."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.ws = {}
        self.tables, self.table_pos, self.pool = [], {}, None

    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _buf(self, name, numel, dtype):
        t = self.ws.get(name)
        if t is None or t.numel() < numel:
            t = self.ws[name] = torch.empty(int(numel), dtype=dtype, device=self.device)
        return t[:int(numel)]

    def _upload(self, name, host):
        t = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
        d = self._buf(name, t.numel(), t.dtype)
        d.copy_(t)
        return d

    def _table(self, n, O):
        """-> (offset in the pool, T) of the (n, O) table, (0, 0) for an axis that keeps its size."""
        if n == O:
            return 0, 0
        pos = self.table_pos.get((n, O))
        if pos is None:
            rows = table_rows(n, O)
            pos = self.table_pos[(n, O)] = (sum(t.size for t in self.tables), rows.shape[1] - 2)
            self.tables.append(rows)
            self.pool = None
        return pos

    def pack(self, frames, size):
        """The ragged batch both resizes take: -> (B, h, w, packed bytes, hw, off, tab_idx, largest tap count), all on the host."""
        h, w = int(size[0]), int(size[1])
        B = len(frames)
        frames = [check_frame(f, "frame %d" % i) for i, f in enumerate(frames)]
        hw = np.array([f.shape[:2] for f in frames], dtype=np.int32)
        off = np.zeros(B, dtype=np.int64)
        pos = 0
        for b, f in enumerate(frames):
            off[b] = pos
            pos += -(-f.size // 16) * 16
        flat = np.zeros(pos, dtype=np.uint8)
        for f, o in zip(frames, off):
            flat[o:o + f.size] = f.reshape(-1)
        idx = np.array([self._table(W, w) + self._table(H, h) for H, W in hw], dtype=np.int32)
        if self.pool is None:
            self.pool = torch.from_numpy(np.concatenate([t.reshape(-1) for t in self.tables] or [np.zeros(1, np.int32)])).to(self.device)
        return B, h, w, flat, hw, off, idx, int(idx[:, (1, 3)].max())

    def imresize(self, frames, size, mean=None, std=None, want_u8=False):
        """[H_b x W_b x 3 uint8 arrays] -> (uint8 [B, h, w, 3] or None, normalised fp32 [B, 3, h, w] or None when mean is None)."""
        B, h, w, flat, hw, off, idx, taps = self.pack(frames, size)
        d_flat, d_hw, d_off, d_idx = (self._upload(n, a) for n, a in (("frames", flat), ("hw", hw), ("off", off), ("tab_idx", idx)))
        minmax = self._buf("minmax", B * IMAGE_CHUNKS * 2, torch.int32)
        u8 = torch.empty((B, h, w, 3), dtype=torch.uint8, device=self.device) if want_u8 else None
        f32 = torch.empty((B, 3, h, w), dtype=torch.float32, device=self.device) if mean is not None else None
        mean_h = (ctypes.c_float * 3)(*mean) if mean is not None else None
        std_h = (ctypes.c_float * 3)(*std) if mean is not None else None
        _lib.call("dn_imresize_u8", d_flat.data_ptr(), d_hw.data_ptr(), d_off.data_ptr(), B, h, w, self.pool.data_ptr(), d_idx.data_ptr(),
                  taps, minmax.data_ptr(), u8.data_ptr() if want_u8 else None, mean_h, std_h,
                  f32.data_ptr() if f32 is not None else None, self.stream())
        return u8, f32

    def workspace(self, name, nbytes):
        """A named uint8 device buffer of at least nbytes that is reused between calls (for callers that pack their own transfers)."""
        return self._buf(name, nbytes, torch.uint8)

    def resize_packed(self, B, h, w, flat, hw, off, idx, taps, out):
        """dn_resize_u8 on a batch pack() made and the caller has uploaded: flat / hw / off / idx / out are device addresses (out: uint8
        [B, h, w, 3]).  The one call site of the entry point."""
        _lib.call("dn_resize_u8", flat, hw, off, B, h, w, self.pool.data_ptr(), idx, taps, out, self.stream())

    def resize(self, frames, size):
        """PIL's Image.fromarray(f).resize((w, h), Image.BILINEAR) of [H_b x W_b x 3 uint8 arrays] -> uint8 [B, h, w, 3] on the device
        (dn_resize_u8: imresize without the byte-scale, what scipy.misc.imresize does to a uint8 frame)."""
        B, h, w, flat, hw, off, idx, taps = self.pack(frames, size)
        d_flat, d_hw, d_off, d_idx = (self._upload(n, a) for n, a in (("frames", flat), ("hw", hw), ("off", off), ("tab_idx", idx)))
        u8 = torch.empty((B, h, w, 3), dtype=torch.uint8, device=self.device)
        self.resize_packed(B, h, w, d_flat.data_ptr(), d_hw.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), taps, u8.data_ptr())
        return u8

    def colorize(self, maps, rect=None, max_value=None, table=None, reciprocal=False):
        """255 * tensor2array(maps[b, r0:r1, c0:c1], max_value, table=table) as uint8 [B, r1-r0, c1-c0, 3] on the device.  maps: fp32
        [B, h, w] on the device; table: uint8 [256, 3] RGB (numpy or a device tensor) or None for the grey branch; reciprocal colours
        1 / maps."""
        assert maps.dim() == 3 and maps.dtype == torch.float32 and maps.is_cuda and maps.is_contiguous()
        B, h, w = maps.shape
        r0, r1, c0, c1 = (0, h, 0, w) if rect is None else rect
        out = torch.empty((B, max(r1 - r0, 0), max(c1 - c0, 0), 3), dtype=torch.uint8, device=self.device)
        d_table = None
        if table is not None:
            d_table = table if torch.is_tensor(table) else self._upload("table", np.asarray(table, dtype=np.uint8).reshape(256, 3))
        ws = self._buf("max", B * IMAGE_CHUNKS, torch.float32)
        _lib.call("dn_colorize_u8", maps.data_ptr(), B, h, w, r0, r1, c0, c1, 1 if reciprocal else 0,
                  -1.0 if max_value is None else float(max_value), d_table.data_ptr() if d_table is not None else None, ws.data_ptr(),
                  out.data_ptr(), self.stream())
        return out

    def contrast(self, images, factor):
        """PIL.ImageEnhance.Contrast(im).enhance(factor) of uint8 [B, h, w, 3] on the device."""
        assert images.dim() == 4 and images.shape[3] == 3 and images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous()
        B, h, w, _ = images.shape
        out = torch.empty_like(images)
        ws = self._buf("lumasum", B * IMAGE_CHUNKS, torch.int64)
        _lib.call("dn_contrast_u8", images.data_ptr(), B, h, w, float(factor), ws.data_ptr(), out.data_ptr(), self.stream())
        return out


def colorize(maps, rect=None, max_value=None, table=None, reciprocal=False):
    """ImageOps.colorize on the device `maps` lives on."""
    return ImageOps(maps.device).colorize(maps, rect, max_value, table, reciprocal)


# ------------------------------------------------------------------------------------------------ the host statement
def host_preprocess(args, frame, mean, std):
    """run_inference.py:121-141 -> normalised fp32 [1, 3, h, w] on the host."""
    img = frame.astype(np.float32)
    h, w, _ = img.shape
    if (not args.no_resize) and (h != args.img_height or w != args.img_width):
        img = KE.imresize_bilinear(img, (args.img_height, args.img_width)).astype(np.float32)
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1))))
    mean, std = torch.tensor(mean).view(3, 1, 1), torch.tensor(std).view(3, 1, 1)
    return ((t / 255 - mean) / std).unsqueeze(0)


def host_images(args, output, tables=None):
    """run_inference.py:157-183 on one network output [1, h, w] (a host tensor) -> {"disp", "en", "depth"} uint8 images (those the flags
    ask for).  tables: {"bone": uint8 [256, 3], "rainbow": ...} instead of OpenCV's."""
    from PIL import Image, ImageEnhance
    from . import utils as U
    tables = tables or {}
    out = {}
    if args.output_disp:
        r0, r1, c0, c1 = garg_rectangle(args.img_height, args.img_width)
        arr = U.tensor2array(output[:, r0:r1, c0:c1], max_value=None, colormap="bone", channel_first=False, table=tables.get("bone"))
        out["disp"] = (255 * arr).astype(np.uint8)
        out["en"] = np.asarray(ImageEnhance.Contrast(Image.fromarray(out["disp"])).enhance(CONTRAST))
    if args.output_depth:
        arr = U.tensor2array(1 / output, max_value=DEPTH_MAX, colormap="rainbow", channel_first=False, table=tables.get("rainbow"))
        out["depth"] = (255 * arr).astype(np.uint8)
    return out


def device_images(args, ops, output, tables=None):
    """host_images for a batch on the device: output fp32 [B, h, w] -> {"disp", "en", "depth"} uint8 numpy arrays [B, ...]."""
    tables = tables or {}
    out = {}
    if args.output_disp:
        disp = ops.colorize(output, garg_rectangle(args.img_height, args.img_width), None, tables.get("bone"))
        out["disp"], out["en"] = disp, ops.contrast(disp, CONTRAST)
    if args.output_depth:
        out["depth"] = ops.colorize(output, None, DEPTH_MAX, tables.get("rainbow"), reciprocal=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the command line
def build_parser():
    p = argparse.ArgumentParser(description="Inference script for DispNet learned with Structure from Motion Learner inference on KITTI "
                                            "and CityScapes Dataset", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--network", default="disp_vgg", type=str, help="network type")
    p.add_argument("--imagenet-normalization", action="store_true", help="use imagenet parameter for normalization.")
    p.add_argument("--monodepth2", action="store_true", help="to inference monodepth2 model")
    p.add_argument("--output-disp", action="store_true", help="save disparity img")
    p.add_argument("--output-depth", action="store_true", help="save depth img")
    p.add_argument("--pretrained", required=True, type=str, help="pretrained DispNet path")
    p.add_argument("--img-height", default=128, type=int, help="Image height")
    p.add_argument("--img-width", default=416, type=int, help="Image width")
    p.add_argument("--no-resize", action="store_true", help="no resizing is done")
    p.add_argument("--dataset-list", default=None, type=str, help="Dataset list file")
    p.add_argument("--dataset-dir", default=".", type=str, help="Dataset directory")
    p.add_argument("--output-dir", default="output", type=str, help="Output directory")
    p.add_argument("--img-exts", default=["png", "jpg", "bmp"], nargs="*", type=str, help="images extensions to glob")
    # extensions (not in the reference)
    p.add_argument("--batch", default=8, type=int, metavar="N", help="images per forward")
    p.add_argument("--readers", default=4, type=int, metavar="K", help="host threads that read files ahead of the GPU (at most 16)")
    p.add_argument("--host-chain", action="store_true",
                   help="the reference's per-image chain: resize, colouring and contrast in numpy / PIL on the host, one image per forward")
    return p


def create_disp_net(args, device):
    """run_inference.py:54-98."""
    from . import models, networks, utils as U
    if args.monodepth2:
        if args.network == "disp_vgg_BN":
            enc = networks.vggEncoder(num_layers=16, pretrained=False).to(device)
        elif args.network == "disp_res_18":
            enc = networks.ResnetEncoder(num_layers=18, pretrained=False).to(device)
        else:
            raise ValueError("undefined network")
        dec = networks.DepthDecoder(enc.num_ch_enc).to(device)
        U.load_model({"encoder": enc, "depth": dec}, args.pretrained)
        return models.monodepth2(encoder=enc, decoder=dec)
    table = {"dispnet": "DispNetS", "disp_res": "Disp_res", "disp_vgg": "Disp_vgg_feature", "disp_vgg_BN": "Disp_vgg_BN", "FCRN": "FCRN",
             "ASPP": "deeplab_depth", "disp_vgg_BN_DORN": "Disp_vgg_BN_DORN"}
    if args.network not in table:
        raise ValueError("undefined network")
    net = getattr(models, table[args.network])().to(device)
    net.load_state_dict(torch.load(args.pretrained, map_location=device)["state_dict"])
    return net


def forward(args, net, img):
    """One eval-mode forward -> the map run_inference.py colours, fp32 [B, h, w] (:143-149)."""
    from . import functional, utils as U
    if args.network in ("DORN", "disp_vgg_BN_DORN"):
        pred_d, _ = net(img)
        output = functional.reciprocal(U.get_depth_sid(pred_d))
    else:
        output = net(img)
    return output.reshape(img.shape[0], output.shape[-2], output.shape[-1]).contiguous().float()


def list_files(args):
    """run_inference.py:108-112 (the glob sorted per extension, so that {j}_disp names do not depend on the directory order)."""
    if args.dataset_list is not None:
        with open(args.dataset_list, "r") as f:
            return [os.path.join(args.dataset_dir, name) for name in f.read().splitlines()]
    return [os.path.join(args.dataset_dir, n) for ext in args.img_exts for n in sorted(os.listdir(args.dataset_dir))
            if n.endswith("." + ext)]


class _Frames(object):
    def __init__(self, files):
        self.files = files

    def __getitem__(self, j):
        from PIL import Image
        with Image.open(self.files[j]) as im:
            return check_frame(np.asarray(im), self.files[j])


def _save(images, j0, files, output_dir):
    from PIL import Image
    written = []
    for kind, batch in images.items():
        for i, arr in enumerate(batch):
            base, ext = os.path.splitext(os.path.basename(files[j0 + i]))
            name = "{}_depth{}".format(base, ext) if kind == "depth" else "{}_{}{}".format(j0 + i, kind, ext)
            Image.fromarray(arr).save(os.path.join(output_dir, name))
            written.append(name)
    return written


@torch.no_grad()
def main(argv=None, tables=None, keep_outputs=False):
    """-> {"output_dir", "files" (names written), "outputs" (the network output [h, w] per image, with keep_outputs)}."""
    args = build_parser().parse_args(argv)
    if not (args.output_disp or args.output_depth):
        print("You must at least output one value !")
        return None
    if args.batch < 1:
        raise SystemExit("run_inference.py: --batch must be >= 1")
    args.readers = max(1, min(MAX_READERS, args.readers))
    if not torch.cuda.is_available():
        raise SystemExit("run_inference.py drives the MI355X HIP path; no GPU is visible (there is no CPU fallback)")
    device = torch.device("cuda")
    from . import utils as U
    from .data import normalization
    net = create_disp_net(args, device)
    net.eval()
    mean, std = normalization(args.imagenet_normalization, args.monodepth2)
    if tables is None:
        tables = {name: U.colour_table(name) for name in ("bone", "rainbow")}
    output_dir = os.path.join(args.output_dir, args.network, datetime.datetime.now().strftime("%m-%d-%H:%M"))
    os.makedirs(output_dir, exist_ok=True)
    files = list_files(args)
    n = len(files)
    print("{} files to test".format(n))
    ops = ImageOps(device)
    batch_size = 1 if args.host_chain else args.batch
    result = {"output_dir": output_dir, "files": [], "outputs": []}
    batch = []
    for j, frame in enumerate(prefetched(_Frames(files), n, args.readers, 2 * batch_size + args.readers)):
        batch.append(frame)
        if len(batch) < batch_size and j < n - 1:
            continue
        j0 = j + 1 - len(batch)
        if args.host_chain:
            output = forward(args, net, host_preprocess(args, batch[0], mean, std).to(device))
            images = {k: v[None] for k, v in host_images(args, output.cpu(), tables).items()}
        else:
            if args.no_resize:
                if any(f.shape != batch[0].shape for f in batch):
                    raise ValueError("--batch needs frames of one size per batch; use --batch 1 with --no-resize on mixed sizes")
                size = batch[0].shape[:2]
            else:
                size = (args.img_height, args.img_width)
            _, img = ops.imresize(batch, size, mean, std)
            output = forward(args, net, img)
            images = device_images(args, ops, output, tables)
        result["files"] += _save(images, j0, files, output_dir)
        if keep_outputs:
            result["outputs"] += list(output.cpu().numpy())
        batch = []
    return result
