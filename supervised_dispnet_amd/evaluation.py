"""Batched evaluation of test_disp.py's chain on the device (eval_disp.py --eval-batch): everything between the
resized input frames and the seven error numbers of an image stays on the GPU -- with --device-resize (KITTI) the resize too: the raw
frames are uploaded and dn_imresize_u8 writes the normalised batch, bit for bit what the host path uploads.

Per batch the host does what test_disp.evaluate_sample does before the forward (scipy.misc.imresize semantics, transpose) and packs
ground truth and masks; the device normalises, runs ONE eval-mode forward at batch B, takes 1/disp (or the SID decode), and then
dn_zoom3_prefilter -> dn_zoom3_clip -> dn_eval_errors.  Ground truths of a batch may differ in size (KITTI: 370x1226, 374x1238,
375x1242, 376x1241), so the zoomed predictions, the ground truth and the masks share one ragged layout: image b is H_b x W_b elements
at element offset off[b], offsets aligned to RAGGED_ALIGN elements.  [B][8] floats come back; the network-resolution depth only when
the caller keeps predictions.

With protocol "monodepth2" (eval_disp.py --protocol monodepth2 [--post-process]) the chain after the forward is
monodepth2's evaluate_depth.py instead: [one forward at 2B and dn_mono2_post_process ->] dn_bilinear_recip_ragged (the disparity resized
bilinearly to each ground-truth size, then inverted) -> dn_eval_errors_clamp (scale first, clamp last).  The mono2_* functions below state
the same arithmetic in numpy, per image: the yardstick of the device chain and the chain that runs without --eval-batch.
"""
import ctypes

import numpy as np
import torch

from . import _lib, kitti_eval as KE

RAGGED_ALIGN = 4          # elements: the mask's 4-byte reads and the fp32 rows' 16 bytes start aligned
SCALE_NONE, SCALE_FIXED, SCALE_MEDIAN = 0, 1, 2
STEREO_SCALE = 5.4        # test_disp.py:394


def ragged_layout(shapes, align=RAGGED_ALIGN):
    """[(H_b, W_b)] -> (hw int32 [B, 2], off int64 [B], npix int32 [B], total elements)."""
    hw = np.asarray(shapes, dtype=np.int32).reshape(-1, 2)
    npix = (hw[:, 0].astype(np.int64) * hw[:, 1]).astype(np.int32)
    off = np.zeros(len(hw), dtype=np.int64)
    pos = 0
    for b, n in enumerate(npix):
        off[b] = pos
        pos += -(-int(n) // align) * align
    return hw, off, npix, pos


def pack_ragged(arrays, dtype, off, total):
    """2-D arrays -> one flat array of `total` elements of `dtype`, array b raveled at off[b] (gaps are zero)."""
    flat = np.zeros(total, dtype=dtype)
    for a, o in zip(arrays, off):
        flat[o:o + a.size] = np.asarray(a).reshape(-1)
    return flat


def unpack_ragged(flat, hw, off):
    return [flat[o:o + int(h) * int(w)].reshape(int(h), int(w)) for (h, w), o in zip(hw, off)]


def numpy_median_f32(a):
    """np.median of a float32 array, spelled out (the rule dn_eval_errors implements): the middle element of the sorted values for an
    odd count, the float32 (a + b) / 2 of the two middle elements for an even one; NaN for none."""
    s = np.sort(np.asarray(a, dtype=np.float32).reshape(-1))
    n = s.size
    if n == 0:
        return np.float32(np.nan)
    lo = s[(n - 1) // 2]
    return lo if n % 2 else np.float32(np.float32(lo + s[n // 2]) / np.float32(2))


def median_scale_f32(gt, pred):
    """The scale of --unsupervised / --mono on float32 arrays: a float32 division of the two medians."""
    return np.float32(numpy_median_f32(gt) / numpy_median_f32(pred))


def scale_mode(args):
    """test_disp.py:391-396 -> (mode, fixed scale)."""
    if args.unsupervised or args.mono:
        return SCALE_MEDIAN, 1.0
    if args.stereo:
        return SCALE_FIXED, STEREO_SCALE
    return SCALE_NONE, 1.0


PROTOCOLS = ("reference", "monodepth2")
SID_NETWORKS = ("DORN", "disp_vgg_BN_DORN")


def check_protocol(protocol, post_process, gt_type="KITTI", network=None):
    """What --protocol monodepth2 covers; a ValueError names the flag that does not fit."""
    if protocol not in PROTOCOLS:
        raise ValueError("--protocol must be one of {}".format(", ".join(PROTOCOLS)))
    if post_process and protocol != "monodepth2":
        raise ValueError("--post-process belongs to monodepth2's evaluation; add --protocol monodepth2")
    if protocol == "monodepth2" and gt_type == "NYU":
        raise ValueError("--protocol monodepth2 is KITTI's evaluation; it does not take --gt-type NYU")
    if protocol == "monodepth2" and network in SID_NETWORKS:
        raise ValueError("--protocol monodepth2 resizes a disparity; --network {} decodes ordinal labels into depth".format(network))


# ---- monodepth2's evaluate_depth.py per image on the host: the arithmetic of dn_mono2_post_process,
# dn_bilinear_recip_ragged and dn_eval_errors_clamp in numpy -- fp64 from the fp32 inputs, rounded where the kernels round.  The
# yardstick of the device chain, and what eval_disp.py --protocol monodepth2 runs without --eval-batch.
def mono2_ramps(w):
    """-> (lm, rm) float64 [w]: lm = 1 - clip(20 (x / (w - 1) - 0.05), 0, 1), rm its mirror; w >= 2."""
    if w < 2:
        raise ValueError("post-processing needs at least two columns")
    lm = 1.0 - np.clip(20.0 * (np.arange(w, dtype=np.float64) / (w - 1) - 0.05), 0.0, 1.0)
    return lm, lm[::-1].copy()


def mono2_post_process(disp, disp_mirrored):
    """disp and the network's output for the mirrored frame (as it came: still mirrored), float32 [h, w] -> float32 [h, w]."""
    L = np.asarray(disp, dtype=np.float32).astype(np.float64)
    R = np.asarray(disp_mirrored, dtype=np.float32).astype(np.float64)[:, ::-1]
    lm, rm = mono2_ramps(L.shape[1])
    return (rm * L + lm * R + (1.0 - lm - rm) * (0.5 * (L + R))).astype(np.float32)


def bilinear_taps(n, O):
    """One axis of the half-pixel bilinear resize n -> O: (i0, i1 int64 [O], f float64 [O]), edges replicated."""
    s = (np.arange(O, dtype=np.float64) + 0.5) * (float(n) / float(O)) - 0.5
    fl = np.floor(s)
    f, i0 = s - fl, fl.astype(np.int64)
    f[i0 < 0] = 0.0
    i0[i0 < 0] = 0
    f[i0 >= n - 1] = 0.0
    i0[i0 >= n - 1] = n - 1
    return i0, np.minimum(i0 + 1, n - 1), f


def mono2_resize_recip(disp, shape):
    """float32 [h, w] -> the depth 1 / resize(disp) as float32 [H, W]: rows blended in x, then the two results in y, one division."""
    d = np.asarray(disp, dtype=np.float32).astype(np.float64)
    y0, y1, fy = bilinear_taps(d.shape[0], int(shape[0]))
    x0, x1, fx = bilinear_taps(d.shape[1], int(shape[1]))
    top = (1.0 - fx) * d[y0][:, x0] + fx * d[y0][:, x1]
    bot = (1.0 - fx) * d[y1][:, x0] + fx * d[y1][:, x1]
    return (1.0 / ((1.0 - fy)[:, None] * top + fy[:, None] * bot)).astype(np.float32)


def mono2_errors(gt, depth, mask, mode, fixed, lo, hi):
    """Steps 4-6 -> (float64 [7], float32 scale): the scale from the unclamped depth, fp32(depth * scale) clamped to [lo, hi], thresholds
    in fp32, the four means in fp64 (dn_eval_errors' rule)."""
    mask = np.asarray(mask, dtype=bool)
    g, p = np.asarray(gt)[mask].astype(np.float32), np.asarray(depth, dtype=np.float32)[mask]
    scale = {SCALE_NONE: np.float32(1), SCALE_FIXED: np.float32(fixed)}.get(mode)
    if g.size == 0:
        return np.full(7, np.nan), np.float32(np.nan) if scale is None else scale
    if scale is None:
        scale = median_scale_f32(g, p)
    ps = np.minimum(np.maximum(p * scale, np.float32(lo)), np.float32(hi))
    thr = np.maximum(g / ps, ps / g)
    gd, pd = g.astype(np.float64), ps.astype(np.float64)
    d, dl = gd - pd, np.log(gd) - np.log(pd)
    return np.array([np.mean(np.abs(d) / gd), np.mean(d * d / gd), np.sqrt(np.mean(d * d)), np.sqrt(np.mean(dl * dl)),
                     np.mean(thr < np.float32(1.25)), np.mean(thr < np.float32(1.5625)), np.mean(thr < np.float32(1.953125))]), scale


def mono2_host_chain(disp, disp_mirrored, gt, mask, mode, fixed, lo, hi):
    """One image, steps 1-6 -> (float64 [7], scale, the disparity the resize took); disp_mirrored None: no post-processing."""
    if disp_mirrored is not None:
        disp = mono2_post_process(disp, disp_mirrored)
    errs, scale = mono2_errors(gt, mono2_resize_recip(disp, np.shape(gt)), mask, mode, fixed, lo, hi)
    return errs, scale, np.asarray(disp, dtype=np.float32)


@torch.no_grad()
def mono2_evaluate_sample(args, disp_net, sample, device, min_depth, max_depth, post_process=False):
    """test_disp.evaluate_sample's place under --protocol monodepth2: the frame prepared and normalised as there, one forward at batch 1
    (2 with post-processing: the frame and its mirror image), the disparity copied back, the host chain above.
    -> (float64 [7], scale, depth 1 / disp at network resolution)."""
    from .data import normalization
    frame = prepare_frame(args, sample)
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(frame, (2, 0, 1)))).float()
    mean, std = normalization(args.imagenet_normalization, args.monodepth2)
    t = ((t / 255 - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)).unsqueeze(0)
    if post_process:
        t = torch.cat([t, torch.flip(t, dims=[3])])
    disp = disp_net(t.to(device)).float().cpu().numpy()[:, 0]
    gt, mask = sample_ground_truth(args, sample, min_depth, max_depth)
    mode, fixed = scale_mode(args)
    errs, scale, used = mono2_host_chain(disp[0], disp[1] if post_process else None, gt, mask, mode, fixed, min_depth, max_depth)
    return errs, scale, np.float32(1) / used


def network_size(args):
    return (256, 352) if args.gt_type == "NYU" else (args.img_height, args.img_width)   # NYU size hard-coded (test_disp.py:154-155)


def prepare_frame(args, sample):
    """The host half of evaluate_sample before the forward: HWC frame, resized like scipy.misc.imresize unless --no-resize or already
    at the network's size.  Returns a uint8 [h, w, 3] array (resized) or a float32 one (untouched)."""
    tgt = sample["tgt"]
    if args.gt_type == "NYU":
        tgt = np.transpose(tgt, (1, 2, 0))
    h, w, _ = tgt.shape
    img_h, img_w = network_size(args)
    if (not args.no_resize) and (h != img_h or w != img_w):
        return np.ascontiguousarray(KE.imresize_bilinear(tgt, (img_h, img_w)))
    return np.ascontiguousarray(tgt, dtype=np.float32)


def raw_frame(sample):
    """The frame as the file holds it, uint8 [H, W, 3], for --device-resize: sample["tgt_u8"] where the framework kept it, else
    sample["tgt"] cast back (refused unless that is exact: the device byte-scales integers)."""
    u8 = sample.get("tgt_u8")
    if u8 is None:
        u8 = sample["tgt"].astype(np.uint8)
        if not np.array_equal(u8, sample["tgt"]):
            raise ValueError("--device-resize takes frames with integer values 0 ... 255")
    return u8


def sample_ground_truth(args, sample, min_depth, max_depth):
    gt = sample["gt_depth"]
    if args.gt_type == "NYU" and gt.ndim == 3:
        gt = gt[0]
    mask = sample["mask"] if args.gt_type == "KITTI" else (gt > min_depth) & (gt < max_depth)
    return gt, mask


def prefetched(source, n, readers, ahead):
    """source[0], source[1], ... in order, read by `readers` threads up to `ahead` items in front of the consumer."""
    import collections
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=readers) as pool:
        pending = collections.deque()
        nxt = 0
        for _ in range(n):
            while nxt < n and len(pending) < ahead:
                pending.append(pool.submit(source.__getitem__, nxt))
                nxt += 1
            yield pending.popleft().result()


class DeviceEvaluator(object):
    """evaluate(samples) -> (errors float32 [7, n], [depth at network resolution] or None per sample).  Workspaces grow to the largest
    batch seen and are reused."""

    def __init__(self, args, disp_net, device, min_depth, max_depth, keep_depth=None, protocol=None, post_process=None):
        from .data import normalization
        self.args, self.net, self.device = args, disp_net, torch.device(device)
        self.lo, self.hi = float(min_depth), float(max_depth)
        self.keep_depth = (args.output_dir is not None) if keep_depth is None else keep_depth
        self.mode, self.fixed = scale_mode(args)
        self.sid = args.network in SID_NETWORKS
        # "monodepth2": evaluate_depth.py's chain in place of test_disp.py's; post_process: its "+pp" rows
        self.protocol = getattr(args, "protocol", "reference") if protocol is None else protocol
        self.post_process = bool(getattr(args, "post_process", False) if post_process is None else post_process)
        check_protocol(self.protocol, self.post_process, args.gt_type, args.network)
        mean, std = normalization(args.imagenet_normalization, args.monodepth2)
        self.mean_h, self.std_h = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        self.mean_d = torch.tensor(mean, dtype=torch.float32, device=self.device)
        self.std_d = torch.tensor(std, dtype=torch.float32, device=self.device)
        self.ws = {}
        self.image_ops = None                 # --device-resize: the frames are resized by dn_imresize_u8 (inference.ImageOps)
        if getattr(args, "device_resize", False) and args.gt_type == "KITTI" and not args.no_resize:
            from .inference import ImageOps
            self.image_ops = ImageOps(self.device)
        self.scales = None                    # the scale each image of the last batch was given

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

    def _normalised(self, frames):
        """[uint8 or float32 HWC frames of one size] -> normalised fp32 [B, 3, h, w] on the device."""
        B = len(frames)
        h, w, _ = frames[0].shape
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError("--eval-batch needs frames of one size per batch; use --eval-batch 1 with --no-resize on mixed sizes")
        st = torch.cuda.current_stream(self.device).cuda_stream
        img = self._buf("img", B * 3 * h * w, torch.float32).view(B, 3, h, w)
        kitti = self.args.gt_type == "KITTI"
        if kitti and all(f.dtype == np.uint8 for f in frames):
            d = self._upload("u8", np.stack(frames))
            _lib.call("dn_u8_normalize_flip", d.data_ptr(), None, B, h, w, 3, self.mean_d.data_ptr(), self.std_d.data_ptr(), self.mean_h,
                      self.std_h, img.data_ptr(), 3 * h * w, h * w, st)
        else:                                 # frames the host did not resize, and NYU (not divided by 255 in the reference)
            chw = np.stack([np.transpose(f.astype(np.float32), (2, 0, 1)) for f in frames])
            d = self._upload("f32", np.ascontiguousarray(chw))
            _lib.call("dn_eval_normalize", d.data_ptr(), B, h * w, 1 if kitti else 0, self.mean_h, self.std_h, img.data_ptr(), st)
        return img

    @torch.no_grad()
    def predict_depth(self, img):
        """One eval-mode forward at batch B -> depth [B, h, w] fp32, contiguous."""
        from . import functional, utils as U
        if self.sid:
            pred_d, _ = self.net(img)
            depth = U.get_depth_sid(pred_d, ordinal_c=self.args.ordinal_c, dataset=self.args.gt_type)
        else:
            depth = functional.reciprocal(self.net(img))
        B = img.shape[0]
        return depth.reshape(B, depth.shape[-2], depth.shape[-1]).contiguous().float()

    def zoom_clip(self, depth, hw, off, total):
        """depth [B, h, w] on the device -> the ragged zoomed, clipped predictions (a view of a reused workspace)."""
        B, h, w = depth.shape
        st = torch.cuda.current_stream(self.device).cuda_stream
        coef = self._buf("coef", B * h * w, torch.float64)
        d_hw, d_off = self._upload("hw", hw), self._upload("off", off)
        zoomed = self._buf("zoomed", total, torch.float32)
        _lib.call("dn_zoom3_prefilter", depth.data_ptr(), B, h, w, coef.data_ptr(), st)
        _lib.call("dn_zoom3_clip", coef.data_ptr(), B, h, w, d_hw.data_ptr(), d_off.data_ptr(), int(hw[:, 0].max()), int(hw[:, 1].max()),
                  self.lo, self.hi, zoomed.data_ptr(), st)
        return zoomed, d_off

    def mirrored(self, img):
        """[N, 3, h, w] -> [2N, 3, h, w]: planes N .. 2N-1 are the same frames mirrored along the width (dn_flip_w over 3N planes with
        every flag set), so that the post-processing costs ONE forward at 2N."""
        N, C, h, w = img.shape
        img = img.contiguous()
        both = self._buf("img2", 2 * N * C * h * w, torch.float32).view(2 * N, C, h, w)
        both[:N].copy_(img)
        flags = self._buf("flip", N * C, torch.uint8)
        flags.fill_(1)
        _lib.call("dn_flip_w", img.data_ptr(), flags.data_ptr(), N * C, h, w, both[N:].data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return both

    @torch.no_grad()
    def forward_disp(self, img):
        """One eval-mode forward -> the disparity [n, h, w] fp32, contiguous."""
        disp = self.net(img)
        return disp.reshape(img.shape[0], disp.shape[-2], disp.shape[-1]).contiguous().float()

    @torch.no_grad()
    def predict_disp(self, img):
        """The disparity monodepth2's chain resizes, [B, h, w] fp32: the forward at B, or with post-processing the forward at 2B (the
        frames and their mirror images) blended by dn_mono2_post_process."""
        if not self.post_process:
            return self.forward_disp(img)
        B = img.shape[0]
        both = self.forward_disp(self.mirrored(img))
        _, h, w = both.shape
        out = self._buf("pp", B * h * w, torch.float32).view(B, h, w)
        _lib.call("dn_mono2_post_process", both.data_ptr(), B, h, w, out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def resize_recip(self, disp, hw, off, total):
        """disp [B, h, w] on the device -> the ragged depths 1 / resize(disp) at the ground-truth sizes (a view of a reused workspace)."""
        B, h, w = disp.shape
        d_hw, d_off = self._upload("hw", hw), self._upload("off", off)
        resized = self._buf("zoomed", total, torch.float32)
        _lib.call("dn_bilinear_recip_ragged", disp.data_ptr(), B, h, w, d_hw.data_ptr(), d_off.data_ptr(), int(hw[:, 0].max()),
                  int(hw[:, 1].max()), resized.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return resized, d_off

    @torch.no_grad()
    def evaluate(self, samples):
        B = len(samples)
        if self.image_ops is not None:
            _, img = self.image_ops.imresize([raw_frame(s) for s in samples], network_size(self.args), list(self.mean_h), list(self.std_h))
        else:
            img = self._normalised([prepare_frame(self.args, s) for s in samples])
        gts, masks = zip(*(sample_ground_truth(self.args, s, self.lo, self.hi) for s in samples))
        hw, off, npix, total = ragged_layout([g.shape for g in gts])
        d_gt = self._upload("gt", pack_ragged(gts, np.float32, off, total))
        d_mask = self._upload("mask", pack_ragged(masks, np.uint8, off, total))
        d_npix = self._upload("npix", npix)
        out = self._buf("out", B * 8, torch.float32)
        st = torch.cuda.current_stream(self.device).cuda_stream
        if self.protocol == "monodepth2":
            disp = self.predict_disp(img)
            resized, d_off = self.resize_recip(disp, hw, off, total)
            _lib.call("dn_eval_errors_clamp", d_gt.data_ptr(), resized.data_ptr(), d_mask.data_ptr(), d_off.data_ptr(), d_npix.data_ptr(), B,
                      self.mode, self.fixed, self.lo, self.hi, out.data_ptr(), st)
            if self.keep_depth:
                from . import functional
                depth = functional.reciprocal(disp)
        else:
            depth = self.predict_depth(img)
            zoomed, d_off = self.zoom_clip(depth, hw, off, total)
            _lib.call("dn_eval_errors", d_gt.data_ptr(), zoomed.data_ptr(), d_mask.data_ptr(), d_off.data_ptr(), d_npix.data_ptr(), B, self.mode,
                      self.fixed, out.data_ptr(), st)
        res = out.view(B, 8).cpu().numpy()
        self.scales = res[:, 7].copy()
        pred = list(depth.cpu().numpy()) if self.keep_depth else [None] * B
        return np.ascontiguousarray(res[:, :7].T), pred
