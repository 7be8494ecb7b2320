"""Mirror of the reference's loss_functions.py on HIP kernels (same function names, argument order and meaning).

Every function below launches kernels of libdispnet_hip.so through the C ABI; there is no PyTorch fallback (CPU tensors
raise).  PyTorch only provides the tensors, the stream and the autograd hand-off.
"""
import torch

from . import _lib
from .engine import _stream, hbm_call, require_cuda

_MAX_DEPTH = {"kitti": 80.0, "nyu": 10.0}


def _max_depth(datasets):
    if datasets not in _MAX_DEPTH:
        raise ValueError("undefined datasets %r" % (datasets,))   # the reference does `raise "undefined datasets"` (a TypeError)
    return _MAX_DEPTH[datasets]


def _f32c(t, what):
    require_cuda(t, what)
    t = t.detach() if not t.requires_grad else t
    return t.contiguous().float()


# ------------------------------------------------------------------------------------------------ masked depth losses
FUSE_MASKED_FWD = True          # A/B + the bitwise test: False = the three launches (+ the fill of the statistics rows)
_FOLD_COUNTERS = {}             # device -> [zeroed int32 tensor, next slot]: last-arrival counters of the fused forward


def _fold_counter(dev):
    """Address of a zero int32 for one fused launch: 64 slots per device handed out round-robin, so that launches that overlap on the
    device (other streams) count in different slots; every launch leaves its slot zero."""
    from . import engine
    rec = engine.TAPE
    if rec is not None and not rec.get("paused"):
        # a launch tape bakes the address in for good: it gets counters of its own (kept alive with the tape), never shared with the eager
        # launches that keep cycling through the 64 slots below -- validation, a second model's loss -- and may overlap with a replay
        ent = rec.get("fold_counters")
        if ent is None:
            with engine.outside_tape_pool():
                ent = rec["fold_counters"] = [torch.zeros(256, dtype=torch.int32, device=dev), 0]
            rec["keep"].append(ent[0])
        if ent[1] >= 256:
            raise RuntimeError("more than 256 fused loss launches in one recorded step")
        ent[1] += 1
        return ent[0].data_ptr() + 4 * (ent[1] - 1)
    ent = _FOLD_COUNTERS.get(dev)
    if ent is None:
        from .engine import outside_tape_pool
        with outside_tape_pool():                    # persistent: not from a launch tape's private pool
            ent = _FOLD_COUNTERS[dev] = [torch.zeros(64, dtype=torch.int32, device=dev), 0]
    ent[1] = (ent[1] + 1) % 64
    return ent[0].data_ptr() + 4 * ent[1]


class _MaskedLoss(torch.autograd.Function):
    """Sum of terms of the masked-loss family (C entry points dn_masked_loss_fwd/_bwd) as ONE autograd node.
    Term i: `groups[i]` runs of equal length over (gts[i], preds[i]), each with its own mask mean; contributes
    weights[i] * mean over its groups.  The kernels accumulate into one device scalar -- no host arithmetic.

    `sync` (a world size > 1): the terms are WHOLE-BATCH means (Multiscale_*: loss_functions.py:232-237 normalises by the valid
    count of the gathered batch) computed one process per GPU: every rank reduces its own pixels to (sum, count, max) statistics,
    the statistics are all-reduced (distributed.exchange_loss_stats) and the division happens afterwards, so the value is the
    reference's whole-batch number on every rank.  The backward then yields world * d(global loss)/d(local prediction): the
    data-parallel optimizer averages the ranks' parameter gradients (1/world folded into Adam), which restores the sum."""

    @staticmethod
    def forward(ctx, max_depth, kind, groups, weights, sync, gts, *preds):
        lib = _lib.load()
        dev = preds[0].device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        saved, cfg, work = [], [], []
        all_stats = torch.empty((sum(groups[:len(preds)]), _lib.LOSS_STATS), dtype=torch.float32, device=dev)
        # one launch per term (dn_masked_loss_fwd_fused: the last-arriving block reduces and divides) where the term allows it; the rows it
        # writes need no zero fill (columns 0-5 are all the backward reads)
        fused = FUSE_MASKED_FWD and sync <= 1 and kind != _lib.LOSS_BERHU and max(groups[:len(preds)]) <= 256
        if not fused:
            _lib.call("dn_fill", all_stats.data_ptr(), 0.0, all_stats.numel(), _stream())
        row = 0
        for i, (gt, pred) in enumerate(zip(gts, preds)):
            require_cuda(pred, "predicted depth")
            require_cuda(gt, "ground-truth depth")
            gtc, pc = gt.contiguous().float(), pred.contiguous()
            if gtc.numel() != pc.numel():
                raise ValueError("gt %s and prediction %s sizes differ" % (tuple(gt.shape), tuple(pred.shape)))
            g = groups[i]
            pixels = pc.numel() // g
            nbytes = lib.dn_masked_loss_workspace_bytes(g, pixels)
            ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
            stats = all_stats[row:row + g]
            row += g
            if sync > 1:
                _lib.call("dn_masked_loss_stats", gtc.data_ptr(), pc.data_ptr(), g, pixels, max_depth, kind, 0, stats.data_ptr(),
                          ws.data_ptr(), nbytes, _stream())
                work.append((gtc, pc, g, pixels, stats, ws, nbytes))
            elif fused:
                hbm_call("dn::masked_stats_fold_kernel", 8 * g * pixels, "dn_masked_loss_fwd_fused", gtc.data_ptr(), pc.data_ptr(), g, pixels, max_depth, kind,
                         weights[i], 0 if i == 0 else 1, stats.data_ptr(), ws.data_ptr(), nbytes, loss.data_ptr(), _fold_counter(dev), _stream())
            else:
                hbm_call("dn::masked_stats_kernel", 8 * g * pixels, "dn_masked_loss_fwd", gtc.data_ptr(), pc.data_ptr(), g, pixels, max_depth, kind, weights[i], 0 if i == 0 else 1,
                          stats.data_ptr(), ws.data_ptr(), nbytes, loss.data_ptr(), _stream())
            saved += [gtc, pc, stats]
            cfg.append((g, pixels, weights[i], pred.shape))
        if sync > 1:
            from .distributed import exchange_loss_stats
            exchange_loss_stats(all_stats, sum_cols=(0, 1, 2), max_cols=(3,))
            if kind == _lib.LOSS_BERHU:
                for gtc, pc, g, pixels, stats, ws, nbytes in work:
                    _lib.call("dn_masked_loss_stats", gtc.data_ptr(), pc.data_ptr(), g, pixels, max_depth, kind, 1, stats.data_ptr(),
                              ws.data_ptr(), nbytes, _stream())
                exchange_loss_stats(all_stats, sum_cols=(0, 2, 4), max_cols=())
            for i, (gtc, pc, g, pixels, stats, ws, nbytes) in enumerate(work):
                _lib.call("dn_masked_loss_finalize", stats.data_ptr(), g, kind, weights[i], 0 if i == 0 else 1, loss.data_ptr(), _stream())
        ctx.save_for_backward(*saved)
        ctx.cfg = (max_depth, kind, cfg, float(max(sync, 1)))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        max_depth, kind, cfg, up = ctx.cfg
        dl = dloss.contiguous().float()
        grads = []
        for i, (g, pixels, weight, shape) in enumerate(cfg):
            gtc, pc, stats = ctx.saved_tensors[3 * i:3 * i + 3]
            dpred = torch.empty(shape, dtype=torch.float32, device=pc.device)
            hbm_call("dn::masked_loss_bwd_kernel", 12 * g * pixels, "dn_masked_loss_bwd", gtc.data_ptr(), pc.data_ptr(), stats.data_ptr(), dl.data_ptr(), g, pixels, max_depth, kind,
                      weight * up, dpred.data_ptr(), _stream())
            grads.append(dpred)
        return (None, None, None, None, None, None) + tuple(grads)


def _scale0(depth):
    """depth[0][:,0] of the reference, handed over as the whole [B,1,H,W] tensor (same memory, no select node)."""
    d0 = depth[0]
    if d0.dim() != 4 or d0.shape[1] != 1:
        raise ValueError("expected depth[0] of shape [B,1,H,W], got %s" % (tuple(d0.shape),))
    return d0


def _per_sample(gt_depth, depth, datasets, kind):
    d0 = _scale0(depth)
    # per-sample means divided by the batch size: exactly shardable over ranks, no exchange needed
    return _MaskedLoss.apply(_max_depth(datasets), kind, [d0.shape[0]], [1.0], 0, [gt_depth], d0)


def l1_loss(gt_depth, depth, datasets):
    """reference loss_functions.py:104-129 (uses scale 0 only: depth[0][:,0])."""
    return _per_sample(gt_depth, depth, datasets, _lib.LOSS_L1)


def l2_loss(gt_depth, depth, datasets):
    """reference loss_functions.py:77-102; its 'nyu' branch is an L1 (line 97) and is reproduced as such."""
    _max_depth(datasets)
    return _per_sample(gt_depth, depth, datasets, _lib.LOSS_L1 if datasets == "nyu" else _lib.LOSS_L2)


def berhu_loss(gt_depth, depth, datasets):
    """reference loss_functions.py:131-161.  The reference's 'nyu' branch lost its for-loop (NameError at :149); here it
    loops like the 'kitti' branch with max depth 10."""
    return _per_sample(gt_depth, depth, datasets, _lib.LOSS_BERHU)


def Scale_invariant_loss(gt_depth, depth, datasets):
    """reference loss_functions.py:163-189."""
    return _per_sample(gt_depth, depth, datasets, _lib.LOSS_SCALE_INV)


# ---------------------------------------------------------------------------------------------------------- pyramids
_PYR_MODE = {"max": 0, "avg": 1, "bilinear": 2}


@torch.no_grad()
def _pyramid(image, mode):
    require_cuda(image, "ground-truth depth")
    cur = image.contiguous().float()
    pyr = [cur]
    for _ in range(3):
        n, h, w = cur.shape
        nxt = torch.empty((n, h // 2, w // 2), dtype=torch.float32, device=cur.device)
        _lib.call("dn_pyramid_down2", cur.data_ptr(), n, h, w, mode, nxt.data_ptr(), _stream())
        pyr.append(nxt)
        cur = nxt
    return pyr


def generate_max_pyramid(image):
    """reference loss_functions.py:191-196"""
    return _pyramid(image, 0)


def generate_avg_pyramid(image):
    """reference loss_functions.py:198-203"""
    return _pyramid(image, 1)


def generate_bilinear_pyramid(image):
    """reference loss_functions.py:205-215"""
    return _pyramid(image, 2)


def _multiscale(gt_list, preds, kind):
    """One mask over the WHOLE batch per scale, weight 1/2^i, max depth hard-coded 80 (reference :229-238)."""
    n = min(len(gt_list), len(preds))
    from .distributed import data_parallel_world
    return _MaskedLoss.apply(80.0, kind, [1] * n, [1.0 / (2 ** i) for i in range(n)], data_parallel_world(), list(gt_list[:n]), *preds[:n])


def Multiscale_L1_loss(gt_depth, depth, pool_type="bilinear"):
    """reference loss_functions.py:217-238"""
    if pool_type not in _PYR_MODE:
        raise ValueError("undefined pool type")
    return _multiscale(_pyramid(gt_depth, _PYR_MODE[pool_type]), depth, _lib.LOSS_L1)


class _UpsampleInt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, mode):
        require_cuda(x, "prediction")
        xc = x.contiguous()
        b, c, h, w = xc.shape
        out = torch.empty((b, c, h * scale, w * scale), dtype=torch.float32, device=xc.device)
        _lib.call("dn_upsample_int_fwd", xc.data_ptr(), b * c, h, w, scale, mode, out.data_ptr(), _stream())
        ctx.cfg = (b * c, h, w, scale, mode, xc.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, h, w, scale, mode, shape = ctx.cfg
        d = dout.contiguous()
        dx = torch.empty(shape, dtype=torch.float32, device=d.device)
        _lib.call("dn_upsample_int_bwd", d.data_ptr(), n, h, w, scale, mode, dx.data_ptr(), _stream())
        return dx, None, None


def Multiscale_FULL_L1_loss(gt_depth, depth, pool_type="bilinear"):
    """reference loss_functions.py:240-257: predictions upsampled to full resolution with F.upsample(mode=pool_type)."""
    modes = {"nearest": 0, "bilinear": 1}
    if pool_type not in modes:
        raise NotImplementedError("F.upsample mode %r" % (pool_type,))
    ups = [_UpsampleInt.apply(d, 2 ** i, modes[pool_type]) for i, d in enumerate(depth)]
    return _multiscale([gt_depth] * len(depth), ups, _lib.LOSS_L1)


def Multiscale_L2_loss(gt_depth, depth):
    """reference loss_functions.py:259-273"""
    return _multiscale(_pyramid(gt_depth, 2), depth, _lib.LOSS_L2)


def Multiscale_berhu_loss(gt_depth, depth):
    """reference loss_functions.py:275-296"""
    return _multiscale(_pyramid(gt_depth, 2), depth, _lib.LOSS_BERHU)


def Multiscale_scale_inv_loss(gt_depth, depth):
    """reference loss_functions.py:298-315"""
    return _multiscale(_pyramid(gt_depth, 2), depth, _lib.LOSS_SCALE_INV)


# -------------------------------------------------------------------------------------------------------- photometric
_ROT = {"euler": 0, "quat": 1}
_PAD = {"zeros": 0, "border": 1}


class _Photometric(torch.autograd.Function):
    """photometric_reconstruction_loss (reference loss_functions.py:317-354) as ONE autograd node over all scales and
    reference images: per (scale, ref) one fused warp+|diff| launch forward and one fused backward launch."""

    @staticmethod
    def forward(ctx, tgt_img, intrinsics, intrinsics_inv, pose, rot, pad, align, n_ref, n_scale, has_mask, *rest):
        refs = rest[:n_ref]
        depths = rest[n_ref:n_ref + n_scale]
        masks = rest[n_ref + n_scale:] if has_mask else [None] * n_scale
        dev = tgt_img.device
        for t in (tgt_img, intrinsics, intrinsics_inv, pose) + tuple(refs) + tuple(depths):
            require_cuda(t, "photometric loss input")
        tgt = tgt_img.contiguous().float()
        refs = [r.contiguous().float() for r in refs]
        K, Kinv = intrinsics.contiguous().float(), intrinsics_inv.contiguous().float()
        posec = pose.contiguous().float()
        B, _, H, W = tgt.shape
        if posec.shape[1] != n_ref:
            raise AssertionError("pose.size(1) != len(ref_imgs)")
        lib = _lib.load()
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        saved = []
        first = True
        for d, m in zip(depths, masks):
            dc = d.contiguous().float()
            b, _, h, w = dc.shape
            if m is not None and tuple(m.shape[2:]) != (h, w):
                raise AssertionError("explainability mask and depth sizes differ")
            f = H // h
            down = float(H) / h
            if f == 1:
                tgt_s, refs_s = tgt, refs
            else:
                tgt_s = torch.empty((B, 3, h, w), dtype=torch.float32, device=dev)
                hbm_call("dn::area_down_kernel", 12 * B * (H * W + h * w), "dn_area_down", tgt.data_ptr(), B * 3, H, W, f, tgt_s.data_ptr(), _stream())
                refs_s = []
                for r in refs:
                    rs = torch.empty((B, 3, h, w), dtype=torch.float32, device=dev)
                    hbm_call("dn::area_down_kernel", 12 * B * (H * W + h * w), "dn_area_down", r.data_ptr(), B * 3, H, W, f, rs.data_ptr(), _stream())
                    refs_s.append(rs)
            mc = m.contiguous().float() if m is not None else None
            nb = lib.dn_warp_blocks(h, w)
            per_ref = []
            for i, rs in enumerate(refs_s):
                proj = torch.empty((B, 12), dtype=torch.float32, device=dev)
                kinv_s = torch.empty((B, 9), dtype=torch.float32, device=dev)
                _lib.call("dn_pose_proj_fwd", posec.data_ptr() + 4 * 6 * i, 6 * n_ref, K.data_ptr(), Kinv.data_ptr(), B, rot, down,
                          proj.data_ptr(), kinv_s.data_ptr(), _stream())
                partial = torch.empty(B * nb, dtype=torch.float32, device=dev)
                mptr = (mc.data_ptr() + 4 * i * h * w) if mc is not None else None
                msb = mc.shape[1] * h * w if mc is not None else 0
                hbm_call("dn::warp_fwd_kernel", 4 * B * h * w * (7 + (1 if mc is not None else 0)), "dn_photometric_fwd", tgt_s.data_ptr(), rs.data_ptr(), dc.data_ptr(), proj.data_ptr(), kinv_s.data_ptr(),
                          mptr, msb, B, h, w, pad, align, 1.0, 0 if first else 1, partial.data_ptr(), loss.data_ptr(), _stream())
                first = False
                per_ref.append((rs, proj, kinv_s))
            saved.append((dc, mc, tgt_s, per_ref, down, h, w))
        ctx.saved = saved
        ctx.cfg = (B, rot, pad, align, n_ref, n_scale, has_mask, K, posec, [d.shape for d in depths],
                   [m.shape if m is not None else None for m in masks])
        return loss

    @staticmethod
    def backward(ctx, dloss):
        B, rot, pad, align, n_ref, n_scale, has_mask, K, posec, dshapes, mshapes = ctx.cfg
        dev = posec.device
        dl = dloss.contiguous().float()
        lib = _lib.load()
        dpose = torch.zeros_like(posec)
        ddepths, dmasks = [], []
        first_pose = [True] * n_ref
        for (dc, mc, tgt_s, per_ref, down, h, w), dshape, mshape in zip(ctx.saved, dshapes, mshapes):
            nb = lib.dn_warp_blocks(h, w)
            dd = torch.empty(dshape, dtype=torch.float32, device=dev)
            dm = torch.zeros(mshape, dtype=torch.float32, device=dev) if mshape is not None else None
            for i, (rs, proj, kinv_s) in enumerate(per_ref):
                dpp = torch.empty((B, nb, 12), dtype=torch.float32, device=dev)
                mptr = (mc.data_ptr() + 4 * i * h * w) if mc is not None else None
                msb = mc.shape[1] * h * w if mc is not None else 0
                dmptr = (dm.data_ptr() + 4 * i * h * w) if dm is not None else None
                hbm_call("dn::warp_bwd_kernel", 4 * B * h * w * (8 + (2 if mc is not None else 0)), "dn_photometric_bwd", tgt_s.data_ptr(), rs.data_ptr(), dc.data_ptr(), proj.data_ptr(), kinv_s.data_ptr(),
                          mptr, msb, B, h, w, pad, align, 1.0, dl.data_ptr(), dd.data_ptr(), 0 if i == 0 else 1, dpp.data_ptr(),
                          dmptr, msb, _stream())
                _lib.call("dn_pose_proj_bwd", posec.data_ptr() + 4 * 6 * i, 6 * n_ref, K.data_ptr(), B, rot, down, dpp.data_ptr(), nb,
                          dpose.data_ptr() + 4 * 6 * i, 6 * n_ref, 0 if first_pose[i] else 1, _stream())
                first_pose[i] = False
            ddepths.append(dd)
            dmasks.append(dm)
        ctx.saved = None
        grads = [None, None, None, dpose, None, None, None, None, None, None] + [None] * n_ref + ddepths
        if has_mask:
            grads += dmasks
        return tuple(grads)


def photometric_reconstruction_loss(tgt_img, ref_imgs, intrinsics, intrinsics_inv, depth, explainability_mask, pose,
                                    rotation_mode='euler', padding_mode='zeros', align_corners=False):
    """reference loss_functions.py:317-354.  `align_corners` is F.grid_sample's flag: the reference passes none, which means
    False on torch >= 1.3 (what its code yields today) and meant True on its pinned torch 1.0.1."""
    if type(explainability_mask) not in [tuple, list]:
        explainability_mask = [explainability_mask]
    if type(depth) not in [list, tuple]:
        depth = [depth]
    n = min(len(depth), len(explainability_mask))          # zip() semantics of the reference
    depth, masks = list(depth[:n]), list(explainability_mask[:n])
    has_mask = all(m is not None for m in masks)
    if not has_mask and any(m is not None for m in masks):
        raise ValueError("explainability masks must be given for every scale or for none")
    args = list(ref_imgs) + depth + (masks if has_mask else [])
    return _Photometric.apply(tgt_img, intrinsics, intrinsics_inv, pose, _ROT[rotation_mode], _PAD[padding_mode],
                              1 if align_corners else 0, len(ref_imgs), n, has_mask, *args)


# ------------------------------------------------------------------------------------------- monodepth2 minimum reprojection
_MAX_REPROJ_FRAMES = 4


def _pose_base(axisangle, translation):
    """The dense [B, F, 6] tensor `axisangle` and `translation` are the two halves of (networks.PoseCNN attaches it to the views it
    returns), or None: the loss then reads the pose through the base's strides and returns ONE gradient for it, without the slice
    nodes -- framework kernels a launch tape cannot see -- in between."""
    base = getattr(axisangle, "_dn_pose_base", None)
    if base is None or getattr(translation, "_dn_pose_base", None) is not base:
        return None
    return base


def _dense(t, what):
    """`t` as a contiguous float32 tensor; the copy that may take is a framework kernel, which a launch tape would miss."""
    require_cuda(t, "min_reprojection_loss: " + what)
    if t.dtype != torch.float32 or not t.is_contiguous():
        from .engine import _not_on_tape
        _not_on_tape("the contiguous float32 copy of %s" % what)
        t = t.contiguous().float()
    return t


class _MinReproj(torch.autograd.Function):
    """min_reprojection_loss as ONE autograd node: F (+ F identity) term launches, one select (+ finalize) forward; two launches per
    source frame and one pose launch backward.  `pose`: None (T given as F matrices in `rest`) or the invert flags of the
    (axisangle, translation) form, whose dense base then is rest[-1]."""

    @staticmethod
    def forward(ctx, tgt_img, disp, K, inv_K, cfg, pose, n_ref, *rest):
        disp_mode, d_lo, d_span, automask, w, align, mean = cfg
        refs, tail = rest[:n_ref], rest[n_ref:]
        tgt, dc = _dense(tgt_img, "tgt_img"), _dense(disp, "disp")
        refs = [_dense(r, "source frame") for r in refs]
        Kc, Kic = _dense(K, "K"), _dense(inv_K, "inv_K")           # (torch.inverse hands out column-major matrices)
        B, C3, H, W = tgt.shape
        if C3 != 3 or tuple(dc.shape) != (B, 1, H, W) or tuple(Kc.shape) != (B, 4, 4) or tuple(Kic.shape) != (B, 4, 4):
            raise ValueError("min_reprojection_loss: tgt_img [B,3,H,W], disp [B,1,H,W], K and inv_K [B,4,4] expected")
        if any(r.shape != tgt.shape for r in refs):
            raise ValueError("min_reprojection_loss: every source frame must have the target's shape")
        dev = tgt.device
        lib = _lib.load()
        if pose is None:
            base, mask = None, 0
            Ts = [_dense(t, "T") for t in tail]
            if any(tuple(t.shape) != (B, 4, 4) for t in Ts):
                raise ValueError("min_reprojection_loss: every T must be [B,4,4]")
        else:
            base = tail[0]
            require_cuda(base, "pose")
            if base.dtype != torch.float32 or not base.is_contiguous() or base.numel() != B * n_ref * 6:
                raise ValueError("min_reprojection_loss: the pose base must be a dense float32 [B, F, 6]")
            mask = sum(1 << f for f, inv in enumerate(pose) if inv)
            Tall = torch.empty((n_ref, B, 4, 4), dtype=torch.float32, device=dev)
            _lib.call("dn_pose_matrix_fwd", base.data_ptr(), 6 * n_ref, 6, 1, base.data_ptr() + 12, 6 * n_ref, 6, 1, B, n_ref, 2, mask,
                      Tall.data_ptr(), _stream())
            Ts = [Tall[f] for f in range(n_ref)]
        n = B * H * W
        nch = (2 if automask else 1) * n_ref
        terms = torch.empty((nch, B, H, W), dtype=torch.float32, device=dev)
        common = (B, H, W)
        tail_args = (align, disp_mode, d_lo, d_span, 1e-7, w)
        for f, r in enumerate(refs):
            if automask:
                hbm_call("dn::reproj_term_kernel", 28 * n, "dn_reproj_term", tgt.data_ptr(), r.data_ptr(), None, None, None, None, *common, 0,
                         *tail_args, terms[f].data_ptr(), _stream())
            hbm_call("dn::reproj_term_kernel", 32 * n, "dn_reproj_term", tgt.data_ptr(), r.data_ptr(), dc.data_ptr(), Kc.data_ptr(), Kic.data_ptr(),
                     Ts[f].data_ptr(), *common, 1, *tail_args, terms[(n_ref if automask else 0) + f].data_ptr(), _stream())
        m = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        sel = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
        partial = torch.empty(lib.dn_reproj_select_blocks(n), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev) if mean else None
        hbm_call("dn::reproj_select_kernel", (4 * nch + 5) * n, "dn_reproj_select", terms.data_ptr(), nch, n, m.data_ptr(), sel.data_ptr(),
                 partial.data_ptr(), loss.data_ptr() if mean else None, _stream())
        ctx.saved = (tgt, refs, dc, Kc, Kic, Ts, sel, base)
        ctx.cfg = (cfg, n_ref, mask, disp.shape)
        ctx.mark_non_differentiable(sel)
        return (loss if mean else m), sel

    @staticmethod
    def backward(ctx, dout, _dsel):
        tgt, refs, dc, Kc, Kic, Ts, sel, base = ctx.saved
        (disp_mode, d_lo, d_span, automask, w, align, mean), n_ref, mask, dshape = ctx.cfg
        B, _, H, W = tgt.shape
        dev = tgt.device
        n = B * H * W
        g = _dense(dout, "the upstream gradient")
        nblk = _lib.load().dn_reproj_blocks(H, W)
        ws = torch.empty(9 * n, dtype=torch.float32, device=dev)
        partial = torch.empty((n_ref, B, nblk, 12), dtype=torch.float32, device=dev)
        ddisp = torch.empty(dshape, dtype=torch.float32, device=dev)
        for f, r in enumerate(refs):
            hbm_call("dn::reproj_bwd_kernel", 120 * n, "dn_reproj_bwd", tgt.data_ptr(), r.data_ptr(), dc.data_ptr(), Kc.data_ptr(), Kic.data_ptr(),
                     Ts[f].data_ptr(), B, H, W, align, disp_mode, d_lo, d_span, 1e-7, w, sel.data_ptr(), (n_ref if automask else 0) + f,
                     g.data_ptr() if mean else None, None if mean else g.data_ptr(), ws.data_ptr(), ddisp.data_ptr(), 0 if f == 0 else 1,
                     partial[f].data_ptr(), _stream())
        if base is None:
            dT = torch.empty((n_ref, B, 4, 4), dtype=torch.float32, device=dev)
            _lib.call("dn_reproj_pose_bwd", partial.data_ptr(), nblk, Kc.data_ptr(), B, n_ref, dT.data_ptr(), None, 0, 0, 0, None, 0, 0, 0, 0,
                      None, None, _stream())
            tail = tuple(dT[f] for f in range(n_ref))
        else:
            dbase = torch.empty_like(base)
            _lib.call("dn_reproj_pose_bwd", partial.data_ptr(), nblk, Kc.data_ptr(), B, n_ref, None, base.data_ptr(), 6 * n_ref, 6, 1,
                      base.data_ptr() + 12, 6 * n_ref, 6, 1, mask, dbase.data_ptr(), dbase.data_ptr() + 12, _stream())
            tail = (dbase,)
        ctx.saved = None
        return (None, ddisp, None, None, None, None, None) + (None,) * n_ref + tail


def min_reprojection_loss(tgt_img, ref_imgs, disp, K, inv_K, T, min_depth=0.1, max_depth=100.0, automask=True, ssim_weight=0.85,
                          align_corners=False, reduction="mean"):
    """monodepth2's per-pixel minimum reprojection loss on the reference's layers (layers.py: disp_to_depth, BackprojectDepth,
    Project3D, SSIM), fused: per source frame f
        r_f = w * SSIM(pred_f, tgt).mean(1) + (1 - w) * |tgt - pred_f|.mean(1),   pred_f = grid_sample(ref_imgs[f], Project3D(
              BackprojectDepth(depth, inv_K), K, T[f]), padding_mode="border", align_corners=align_corners)
    and, with `automask`, the same term i_f of the unwarped source frame; m = min over [i_0 .. i_{F-1}, r_0 .. r_{F-1}] (a tie goes to
    the lowest index, so identity terms win ties; monodepth2's random tie-breaker is not reproduced: the function is deterministic).
    depth = disp_to_depth(disp, min_depth, max_depth)[1]; with min_depth=None `disp` IS the depth.  Returns m.mean(), or m [B,1,H,W]
    for reduction="none"; the uint8 map of the winning channel rides on the result as `._dn_selection`.
    `T`: F matrices [B,4,4], or (axisangle, translation, invert_flags) as networks.PoseCNN returns them ([B,F,1,3] each) with one flag
    per frame (transformation_from_parameters's `invert`).  Gradients: disp and T (the pose); a pixel whose minimum is an identity
    term carries none.  `align_corners` is F.grid_sample's flag, False being today's torch default (as in inverse_warp)."""
    refs = list(ref_imgs)
    n_ref = len(refs)
    if not 1 <= n_ref <= _MAX_REPROJ_FRAMES:
        raise ValueError("min_reprojection_loss takes 1 to %d source frames, got %d" % (_MAX_REPROJ_FRAMES, n_ref))
    if reduction not in ("mean", "none"):
        raise ValueError("reduction must be 'mean' or 'none'")
    if min_depth is None:
        depth_cfg = (0, 0.0, 0.0)
    else:
        depth_cfg = (1, 1.0 / max_depth, 1.0 / min_depth - 1.0 / max_depth)
    cfg = depth_cfg + (bool(automask), float(ssim_weight), 1 if align_corners else 0, reduction == "mean")
    pose, tail = None, None
    if isinstance(T, (tuple, list)) and len(T) == 3 and isinstance(T[2], (tuple, list)) and not torch.is_tensor(T[2]):
        axisangle, translation, flags = T
        if len(flags) != n_ref or axisangle.shape[1] != n_ref or translation.shape[1] != n_ref:
            raise ValueError("min_reprojection_loss: one pose and one invert flag per source frame expected")
        base = _pose_base(axisangle, translation)
        if base is not None:
            pose, tail = tuple(bool(f) for f in flags), [base]
        else:
            from .layers import transformation_from_parameters
            tail = [transformation_from_parameters(axisangle[:, f], translation[:, f], invert=bool(flags[f])) for f in range(n_ref)]
    else:
        tail = list(T)
        if len(tail) != n_ref:
            raise ValueError("min_reprojection_loss: %d source frames but %d transformations" % (n_ref, len(tail)))
    out, sel = _MinReproj.apply(tgt_img, disp, K, inv_K, cfg, pose, n_ref, *(refs + tail))
    out._dn_selection = sel
    return out


# --------------------------------------------------------------------------------------- monodepth2's multi-scale objective
_MAX_MONO2_SCALES = 4


def _pose_view(v, base, what):
    """(element offset into `base`, batch / frame / element strides) of a [B, F, 1, 3] view of the pose tensor `base`"""
    if v.dim() != 4 or v.shape[2] != 1 or v.shape[3] != 3 or v.dtype != torch.float32:
        raise ValueError("monodepth2_loss: %s must be a float32 [B, F, 1, 3] view of the pose, got %s" % (what, tuple(v.shape)))
    off = (v.data_ptr() - base.data_ptr()) // 4
    return (off, v.stride(0), v.stride(1), v.stride(3))


class _Mono2(torch.autograd.Function):
    """monodepth2_loss as ONE autograd node.  Forward: (the pose launch,) F identity launches, F warped launches over all scales, one
    select, the means, the smoothness (which leaves its gradient behind), one finalize.  Backward: two launches per source frame over
    all scales, the pose launch and the gather into the coarse maps.  No count depends on the number of scales.
    rest = disps (n_scale), source frames (n_ref), then the F matrices or the pose base."""

    @staticmethod
    def forward(ctx, tgt_img, K, inv_K, cfg, pose, n_ref, n_scale, *rest):
        d_lo, d_span, automask, w, align, smoothness, weights = cfg
        S = n_scale
        disps, refs, tail = rest[:S], rest[S:S + n_ref], rest[S + n_ref:]
        tgt = _dense(tgt_img, "tgt_img")
        dcs = [_dense(d, "the disparity of scale %d" % s) for s, d in enumerate(disps)]
        refs = [_dense(r, "source frame") for r in refs]
        Kc, Kic = _dense(K, "K"), _dense(inv_K, "inv_K")
        B, _, H, W = tgt.shape
        dev = tgt.device
        lib = _lib.load()
        st = _stream()
        if pose is None:
            base, mask, views = None, 0, None
            Ts = [_dense(t, "T") for t in tail]
            if any(tuple(t.shape) != (B, 4, 4) for t in Ts):
                raise ValueError("monodepth2_loss: every T must be [B,4,4]")
        else:
            base = tail[0]
            flags, va, vt = pose
            views = va + vt
            mask = sum(1 << f for f, inv in enumerate(flags) if inv)
            Tall = torch.empty((n_ref, B, 4, 4), dtype=torch.float32, device=dev)
            _lib.call("dn_pose_matrix_fwd", base.data_ptr() + 4 * va[0], va[1], va[2], va[3], base.data_ptr() + 4 * vt[0], vt[1], vt[2], vt[3],
                      B, n_ref, 2, mask, Tall.data_ptr(), st)
            Ts = [Tall[f] for f in range(n_ref)]
        n = B * H * W
        dptr = [d.data_ptr() for d in dcs] + [None] * (_MAX_MONO2_SCALES - S)
        tail_args = (align, d_lo, d_span, 1e-7, w)
        ident = torch.empty((n_ref, B, H, W), dtype=torch.float32, device=dev) if automask else None
        warped = torch.empty((S, n_ref, B, H, W), dtype=torch.float32, device=dev)
        for f, r in enumerate(refs):
            if automask:         # the identity terms do not depend on the scale: once per frame, the launch of min_reprojection_loss
                hbm_call("dn::reproj_term_kernel", 28 * n, "dn_reproj_term", tgt.data_ptr(), r.data_ptr(), None, None, None, None, B, H, W, 0,
                         align, 1, d_lo, d_span, 1e-7, w, ident[f].data_ptr(), st)
            hbm_call("dn::mono2_term_kernel", 32 * n * S, "dn_mono2_term", tgt.data_ptr(), r.data_ptr(), *dptr, Kc.data_ptr(), Kic.data_ptr(),
                     Ts[f].data_ptr(), B, H, W, S, *tail_args, warped[0, f].data_ptr(), n_ref * n, st)
        sel = torch.empty((S, B, 1, H, W), dtype=torch.uint8, device=dev)
        partial = torch.empty(S * lib.dn_mono2_blocks(n), dtype=torch.float32, device=dev)
        nch = (2 if automask else 1) * n_ref
        hbm_call("dn::mono2_select_kernel", (4 * nch + 1) * n * S, "dn_mono2_select", ident.data_ptr() if automask else None,
                 n_ref if automask else 0, warped.data_ptr(), n_ref, S, n, None if weights is None else weights.data_ptr(), sel.data_ptr(),
                 partial.data_ptr(), st)
        tiles = lib.dn_mono2_tiles(H, W)
        mu = torch.empty(S * B, dtype=torch.float32, device=dev)
        smp = torch.empty(S * B * tiles * 2, dtype=torch.float32, device=dev)
        gbuf = torch.empty(sum(d.numel() for d in dcs), dtype=torch.float32, device=dev)
        dotp = torch.empty(S * B * tiles, dtype=torch.float32, device=dev)
        parts = torch.empty((S, 2), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        hbm_call("dn::mono2_smooth_kernel", 16 * n, "dn_mono2_finish_fwd", tgt.data_ptr(), *dptr, B, H, W, S, partial.data_ptr(), smoothness,
                 mu.data_ptr(), smp.data_ptr(), gbuf.data_ptr(), dotp.data_ptr(), parts.data_ptr(), loss.data_ptr(), st)
        ctx.saved = (tgt, refs, dcs, Kc, Kic, Ts, sel, base, (mu, gbuf, dotp), weights)
        ctx.cfg = (cfg, n_ref, mask, views, [d.shape for d in disps])
        ctx.mark_non_differentiable(parts, sel)
        return loss, parts, sel

    @staticmethod
    def backward(ctx, dout, _dparts, _dsel):
        tgt, refs, dcs, Kc, Kic, Ts, sel, base, (mu, gbuf, dotp), weights = ctx.saved
        (d_lo, d_span, automask, w, align, smoothness, _), n_ref, mask, views, shapes = ctx.cfg
        S = len(dcs)
        B, _, H, W = tgt.shape
        dev = tgt.device
        n = B * H * W
        st = _stream()
        g = _dense(dout, "the upstream gradient")
        nblk = _lib.load().dn_reproj_blocks(H, W)
        dptr = [d.data_ptr() for d in dcs] + [None] * (_MAX_MONO2_SCALES - S)
        ws = torch.empty(S * 9 * n, dtype=torch.float32, device=dev)
        ddfull = torch.empty(S * n, dtype=torch.float32, device=dev)
        partial = torch.empty((n_ref, B, S * nblk, 12), dtype=torch.float32, device=dev)
        for f, r in enumerate(refs):
            hbm_call("dn::mono2_bwd_kernel", 120 * n * S, "dn_mono2_bwd", tgt.data_ptr(), r.data_ptr(), *dptr, Kc.data_ptr(), Kic.data_ptr(),
                     Ts[f].data_ptr(), B, H, W, S, align, d_lo, d_span, 1e-7, w, sel.data_ptr(), (n_ref if automask else 0) + f, g.data_ptr(),
                     None if weights is None else weights.data_ptr(), ws.data_ptr(), ddfull.data_ptr(), 0 if f == 0 else 1,
                     partial[f].data_ptr(), st)
        if base is None:
            dT = torch.empty((n_ref, B, 4, 4), dtype=torch.float32, device=dev)
            _lib.call("dn_reproj_pose_bwd", partial.data_ptr(), S * nblk, Kc.data_ptr(), B, n_ref, dT.data_ptr(), None, 0, 0, 0, None, 0, 0, 0, 0,
                      None, None, st)
            tail = tuple(dT[f] for f in range(n_ref))
        else:
            dbase = torch.empty_like(base)
            _lib.call("dn_reproj_pose_bwd", partial.data_ptr(), S * nblk, Kc.data_ptr(), B, n_ref, None, base.data_ptr() + 4 * views[0], views[1],
                      views[2], views[3], base.data_ptr() + 4 * views[4], views[5], views[6], views[7], mask, dbase.data_ptr() + 4 * views[0],
                      dbase.data_ptr() + 4 * views[4], st)
            tail = (dbase,)
        outs = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes]
        optr = [o.data_ptr() for o in outs] + [None] * (_MAX_MONO2_SCALES - S)
        hbm_call("dn::mono2_disp_grad_kernel", 10 * n, "dn_mono2_disp_grad", B, H, W, S, mu.data_ptr(), g.data_ptr(), smoothness, ddfull.data_ptr(),
                 gbuf.data_ptr(), dotp.data_ptr(), *optr, st)
        ctx.saved = None
        return (None,) * 7 + tuple(outs) + (None,) * n_ref + tail


def monodepth2_loss(tgt_img, ref_imgs, disps, K, inv_K, T, min_depth=0.1, max_depth=100.0, scaled_disp=False, automask=True,
                    ssim_weight=0.85, smoothness=1e-3, align_corners=False, _pixel_weights=None):
    """monodepth2's training objective over the S = len(disps) scales of the decoder, disps[s] [B,1,H>>s,W>>s] (S from 1 to 4, H and W
    divisible by 2^(S-1)), fused.  Per scale s:
        up_s    = F.interpolate(disps[s], (H, W), mode="bilinear", align_corners=False)                    (up_0 = disps[0])
        depth_s = 1 / up_s  (scaled_disp=True: networks.DepthDecoder already emits 0.01 + 9.99 sigma)  or  disp_to_depth(up_s, min_depth,
                  max_depth)[1]
        m_s     = the per-pixel minimum over [i_0 .. i_{F-1}, r_{s,0} .. r_{s,F-1}] of min_reprojection_loss (a tie goes to the lowest
                  index; the identity terms i_f of `automask` do not depend on s and are computed once)
        norm_s  = disps[s] / (disps[s].mean((2, 3), keepdim=True) + 1e-7)
        loss    = (1 / S) * sum_s [ m_s.mean() + smoothness / 2^s * get_smooth_loss(norm_s, colour_s) ]
    with colour_s the 2^s x 2^s box average of tgt_img (F.interpolate(mode="area")).  A direction in which a map has no neighbour pair
    (a map one pixel high or wide) contributes 0 to its smoothness, where the mean of an empty tensor would be NaN.
    tgt_img, ref_imgs, K, inv_K, T (F matrices, or (axisangle, translation, invert_flags)) and align_corners (the sampler's flag; the
    upsampling is always align_corners=False) are min_reprojection_loss's.  Returns the scalar; `._dn_parts` [S,2] holds the
    reprojection mean and the unweighted smoothness per scale (device tensor: logging without a sync), `._dn_selection` the S uint8
    maps of the winning channel.  Gradients: every disps[s] and T (the pose).  Deterministic: every sum has a fixed order.
    `_pixel_weights` ([S,B,1,H,W], the fp64 audit's handle): m_s.mean() becomes (m_s * _pixel_weights[s]).mean()."""
    refs, disps = list(ref_imgs), list(disps)
    n_ref, S = len(refs), len(disps)
    if not 1 <= n_ref <= _MAX_REPROJ_FRAMES:
        raise ValueError("monodepth2_loss takes 1 to %d source frames, got %d" % (_MAX_REPROJ_FRAMES, n_ref))
    if not 1 <= S <= _MAX_MONO2_SCALES:
        raise ValueError("monodepth2_loss takes 1 to %d disparity maps, got %d" % (_MAX_MONO2_SCALES, S))
    if tgt_img.dim() != 4 or tgt_img.shape[1] != 3:
        raise ValueError("monodepth2_loss: tgt_img [B,3,H,W] expected")
    B, _, H, W = tgt_img.shape
    if H < 2 or W < 2 or H % (1 << (S - 1)) or W % (1 << (S - 1)):
        raise ValueError("monodepth2_loss: %d x %d is not divisible by 2^%d" % (H, W, S - 1))
    for s, d in enumerate(disps):
        if tuple(d.shape) != (B, 1, H >> s, W >> s):
            raise ValueError("monodepth2_loss: disps[%d] must be %s, got %s" % (s, (B, 1, H >> s, W >> s), tuple(d.shape)))
    if any(r.shape != tgt_img.shape for r in refs):
        raise ValueError("monodepth2_loss: every source frame must have the target's shape")
    if tuple(K.shape) != (B, 4, 4) or tuple(inv_K.shape) != (B, 4, 4):
        raise ValueError("monodepth2_loss: K and inv_K [B,4,4] expected")
    if scaled_disp:
        d_lo, d_span = 0.0, 1.0
    else:
        d_lo, d_span = 1.0 / max_depth, 1.0 / min_depth - 1.0 / max_depth
    weights = None
    if _pixel_weights is not None:
        weights = _dense(_pixel_weights.detach(), "_pixel_weights")
        if tuple(weights.shape) != (S, B, 1, H, W):
            raise ValueError("monodepth2_loss: _pixel_weights must be [S,B,1,H,W]")
    cfg = (d_lo, d_span, bool(automask), float(ssim_weight), 1 if align_corners else 0, float(smoothness), weights)
    pose = None
    if isinstance(T, (tuple, list)) and len(T) == 3 and isinstance(T[2], (tuple, list)) and not torch.is_tensor(T[2]):
        axisangle, translation, flags = T
        if len(flags) != n_ref or axisangle.shape[1] != n_ref or translation.shape[1] != n_ref or axisangle.shape[0] != B:
            raise ValueError("monodepth2_loss: one pose and one invert flag per source frame expected")
        base = _pose_base(axisangle, translation)
        if base is not None:
            require_cuda(base, "pose")
            if base.dtype != torch.float32 or not base.is_contiguous() or base.numel() != B * n_ref * 6:
                raise ValueError("monodepth2_loss: the pose base must be a dense float32 tensor of B * F * 6 elements")
            pose = (tuple(bool(f) for f in flags), _pose_view(axisangle, base, "axisangle"), _pose_view(translation, base, "translation"))
            tail = [base]
        else:
            from .layers import transformation_from_parameters
            tail = [transformation_from_parameters(axisangle[:, f], translation[:, f], invert=bool(flags[f])) for f in range(n_ref)]
    else:
        tail = list(T)
        if len(tail) != n_ref:
            raise ValueError("monodepth2_loss: %d source frames but %d transformations" % (n_ref, len(tail)))
    out, parts, sel = _Mono2.apply(tgt_img, K, inv_K, cfg, pose, n_ref, S, *(disps + refs + tail))
    out._dn_parts = parts
    out._dn_selection = [sel[s] for s in range(S)]
    return out


class _Explainability(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *masks):
        dev = masks[0].device
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        saved = []
        lib = _lib.load()
        for i, m in enumerate(masks):
            require_cuda(m, "explainability mask")
            mc = m.contiguous().float()
            partial = torch.empty(lib.dn_reduce1d_blocks(mc.numel()), dtype=torch.float32, device=dev)
            _lib.call("dn_explainability_fwd", mc.data_ptr(), mc.numel(), 1.0, 0 if i == 0 else 1, partial.data_ptr(), loss.data_ptr(), _stream())
            saved.append(mc)
        ctx.save_for_backward(*saved)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dl = dloss.contiguous().float()
        out = []
        for mc in ctx.saved_tensors:
            g = torch.empty_like(mc)
            _lib.call("dn_explainability_bwd", mc.data_ptr(), dl.data_ptr(), mc.numel(), g.data_ptr(), _stream())
            out.append(g)
        return tuple(out)


def explainability_loss(mask):
    """reference loss_functions.py:357-364: sum over scales of binary_cross_entropy(mask, ones)."""
    if type(mask) not in [tuple, list]:
        mask = [mask]
    return _Explainability.apply(*mask)


# --------------------------------------------------------------------------------------------------------- smoothness
class _Smooth(torch.autograd.Function):
    """loss_functions.py:367-386 for a list of [B,C,H,W] maps (each channel treated as its own map)."""

    @staticmethod
    def forward(ctx, weight_decay, *maps):
        dev = maps[0].device
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        saved, cfg, w = [], [], 1.0
        lib = _lib.load()
        for m in maps:
            require_cuda(m, "prediction map")
            mc = m.contiguous()
            b, c, h, wd = mc.shape
            nb = lib.dn_smooth_blocks(b * c, h, wd)
            partial = torch.empty((nb, 4), dtype=torch.float32, device=dev)
            hbm_call("dn::smooth2_fwd_kernel", 4 * b * c * h * wd, "dn_smooth2_fwd", mc.data_ptr(), b * c, h, wd, w, partial.data_ptr(), loss.data_ptr(), _stream())
            saved.append(mc)
            cfg.append((b * c, h, wd, w))
            w /= weight_decay
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dl = dloss.contiguous().float()
        grads = []
        for mc, (bc, h, wd, w) in zip(ctx.saved_tensors, ctx.cfg):
            g = torch.empty_like(mc)
            hbm_call("dn::smooth2_bwd_kernel", 8 * bc * h * wd, "dn_smooth2_bwd", mc.data_ptr(), dl.data_ptr(), bc, h, wd, w, g.data_ptr(), _stream())
            grads.append(g)
        return (None,) + tuple(grads)


def smooth_loss(pred_map):
    """reference loss_functions.py:367-386: second-order differences, per-scale weight 1, 1/2.3, 1/2.3^2, ..."""
    if type(pred_map) not in [tuple, list]:
        pred_map = [pred_map]
    return _Smooth.apply(2.3, *pred_map)


def smooth_DORN_loss(pred_map):
    """reference loss_functions.py:388-399 (single map, all K channels in one mean)."""
    return _Smooth.apply(2.3, pred_map)


# --------------------------------------------------------------------------------------------------------------- DORN
class _OrdinalLoss(torch.autograd.Function):
    """DORN_loss as one autograd node.  `sync` (a world size > 1): the loss is a WHOLE-BATCH mean (loss_functions.py:69-73 divide by
    the valid-pixel count of the batch the reference's DataParallel gathered on GPU0): every rank reduces its own pixels to
    (sum, count), the pair is summed over the ranks (distributed.exchange_loss_stats) and the division happens afterwards
    (dn_ordinal_loss_finalize); the backward yields world * d(global loss)/d(local probabilities), which the data-parallel
    optimizer's 1/world turns back into the sum -- the same scheme as _MaskedLoss."""

    @staticmethod
    def forward(ctx, gt_depth, ord_labels, target, max_depth, sync=0):
        require_cuda(ord_labels, "ordinal probabilities")
        require_cuda(gt_depth, "ground-truth depth")
        require_cuda(target, "SID target labels")
        oc = ord_labels.contiguous().float()
        n, k, h, w = oc.shape
        gtc = gt_depth.contiguous().float()
        tc = target.contiguous().to(torch.int32)
        if gtc.numel() != n * h * w or tc.numel() != n * h * w:
            raise ValueError("gt_depth / target must be [N,H,W] matching ord_labels [N,K,H,W]")
        dev = oc.device
        nb = _lib.load().dn_ordinal_loss_blocks(n, h * w)
        partial = torch.empty((nb, 2), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("dn_ordinal_loss_fwd", oc.data_ptr(), gtc.data_ptr(), tc.data_ptr(), n, h * w, k, max_depth, partial.data_ptr(),
                  stats.data_ptr(), loss.data_ptr(), _stream())
        if sync > 1:
            from .distributed import exchange_loss_stats
            exchange_loss_stats(stats.view(1, 2), sum_cols=(0, 1))
            _lib.call("dn_ordinal_loss_finalize", stats.data_ptr(), loss.data_ptr(), _stream())
        ctx.save_for_backward(oc, gtc, tc, stats)
        ctx.cfg = (n, k, h, w, max_depth, float(max(sync, 1)))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        oc, gtc, tc, stats = ctx.saved_tensors
        n, k, h, w, max_depth, up = ctx.cfg
        dl = dloss.contiguous().float()
        dord = torch.empty_like(oc)
        _lib.call("dn_ordinal_loss_bwd", oc.data_ptr(), gtc.data_ptr(), tc.data_ptr(), stats.data_ptr(), dl.data_ptr(), n, h * w, k,
                  max_depth, up, dord.data_ptr(), _stream())
        return None, dord, None, None, None


def DORN_loss(gt_depth, ord_labels, target, datasets):
    """reference loss_functions.py:16-74.  Under one process per GPU the (sum, num_valid) pair is exchanged before the division, so the
    value and the gradients are the reference's whole-batch ones."""
    from .distributed import data_parallel_world
    return _OrdinalLoss.apply(gt_depth, ord_labels, target, _max_depth(datasets), data_parallel_world())


# ------------------------------------------------------------------------------------------------------------ metrics
@torch.no_grad()
def compute_errors(gt, pred, dataset='kitti', crop=True, unsupervised=False):
    """reference loss_functions.py:401-448 -> [abs_diff, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3] (python floats)."""
    require_cuda(pred, "predicted depth")
    require_cuda(gt, "ground-truth depth")
    b, h, w = gt.shape
    if dataset == 'kitti':
        # (the reference leaves max_depth undefined for crop=False, loss_functions.py:411-417; 80 is what it means)
        mx = 80.0
        y1, y2, x1, x2 = (int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)) if crop else (0, h, 0, w)
    else:
        mx = 10.0
        y1, y2, x1, x2 = 0, h, 0, w
    gtc, pc = gt.contiguous().float(), pred.contiguous().float()
    scratch = torch.empty((b, 11), dtype=torch.float32, device=pc.device)
    out = torch.empty(8, dtype=torch.float32, device=pc.device)
    _lib.call("dn_compute_errors", gtc.data_ptr(), pc.data_ptr(), b, h, w, mx, y1, y2, x1, x2, 1 if unsupervised else 0,
              scratch.data_ptr(), out.data_ptr(), _stream())
    return out.tolist()
