"""Test-side restatement of monodepth2's ResNet pose network (networks.PoseResnet).  No tests in here.

  * closed-form inputs and weights (oracle.detgen): no RNG, the golden generator and the tests regenerate the same bits;
  * the reference's PoseDecoder.forward (networks/pose_decoder.py:35-54) as functional torch on a state dict, and the pair encoder
    through oracle.nets_res.resnet_encoder -- runnable in fp64 and fp32;
  * the decoder's tail alone, `scale * mean_hw(conv1x1(x) + b)`, composed as the reference composes it (conv, mean(3).mean(2), scale);
  * the tail kernels' error bounds.  They are DERIVED, not measured: with u = 2^-24 (fp32 unit roundoff), every result is a sum of
    products evaluated with at most n rounded operations on any path, so its error is at most n * u * (sum of the absolute values of the
    fp64 terms), first order in u; SAFETY = 1.01 covers the higher orders (n * u < 1e-4 here).  The operation counts:
      out    HW - 1 additions and one division for the mean, C multiply-adds for the product, the bias, the scale   <= HW + C + 3
      dx     O_used multiply-adds, the division scale / HW, the final product                                        <= O_used + 2
      dw     the mean's HW (it is an input of the product), P multiply-adds, the scale                              <= P + HW + 3
      dbias  P - 1 additions, the scale                                                                              <= P + 1
    `scale` is the fp32 value the kernel is handed (TAIL_SCALE = float32(0.01) widened), so the references evaluate the same function.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detgen, nets_res

U = 2.0 ** -24
SAFETY = 1.01
TAIL_SCALE = float(np.float32(0.01))

# (P, HW, C): the smallest shapes at which the tail can go wrong (tests/test_gpu_pose_net.py says what each is for)
TAIL_SHAPES = [(1, 1, 256), (2, 7, 256), (5, 15, 256), (3, 52, 256), (3, 120, 256), (130, 52, 256), (2, 52, 64), (2, 52, 512)]
TAIL_ROWS = [(6, 6), (12, 6), (18, 6)]          # (O, O_used)
TAIL_CASES = [s + r for s in TAIL_SHAPES for r in TAIL_ROWS]


def _binades(shape, tag, lo=-2, hi=2):
    """2^k with k uniform in {lo..hi}: magnitudes spanning a few binades"""
    k = torch.floor(detgen.uniform(shape, tag, lo, hi + 1, torch.float64))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), k)


@functools.lru_cache(maxsize=None)
def tail_inputs(P, HW, C, O, O_used):
    """fp32-representable inputs held as fp64: x [P, C, HW, 1] (NCHW) non-negative with exact zeros (a ReLU output), w [O, C, 1, 1] and
    dout [P, O_used] of mixed sign (cancellation), bias [O]; magnitudes over a few binades."""
    tag = "posetail:%d:%d:%d:%d:%d:" % (P, HW, C, O, O_used)
    x = torch.clamp(detgen.uniform((P, C, HW, 1), tag + "x", -0.4, 1.0, torch.float64), min=0.0) * _binades((P, C, HW, 1), tag + "xb")
    w = detgen.uniform((O, C, 1, 1), tag + "w", -1.0, 1.0, torch.float64) * _binades((O, C, 1, 1), tag + "wb", -3, 0)
    b = detgen.uniform((O,), tag + "b", -0.5, 0.5, torch.float64)
    dout = detgen.uniform((P, O_used), tag + "g", -1.0, 1.0, torch.float64) * _binades((P, O_used), tag + "gb")
    x, w, b, dout = (t.float().double() for t in (x, w, b, dout))
    assert int((x == 0).sum()) > 0 and float(w.min()) < 0 < float(w.max()) and float(dout.min()) < 0 <= float(dout.max())
    return dict(x=x, w=w, b=b, dout=dout, O_used=O_used, scale=TAIL_SCALE)


def tail_composed(i, dtype, mean_first=False):
    """The tail as the reference composes it (pose_decoder.py:43-49: the 1x1 conv over every pixel, mean(3).mean(2), the scale), all O
    rows evaluated and the first O_used read; autograd under dout.  -> dict(out [P, O_used], dx [P, C, HW, 1], dw, dbias).
    mean_first: the same function with the mean taken before the product, the order the bounds count operations for."""
    x, w, b = (i[k].to(dtype).clone().requires_grad_() for k in ("x", "w", "b"))
    if mean_first:
        out = (i["scale"] * (x.mean(3).mean(2) @ w.reshape(w.shape[0], -1).t() + b))[:, :i["O_used"]]
    else:
        out = (i["scale"] * F.conv2d(x, w, b).mean(3).mean(2))[:, :i["O_used"]]
    (out * i["dout"].to(dtype)).sum().backward()
    return dict(out=out.detach(), dx=x.grad, dw=w.grad, dbias=b.grad)


def tail_bounds(i, dbias_ops=None):
    """The derived bounds (module docstring), fp64, shaped like tail_composed's results.  dbias_ops: the operation count of the bias
    gradient when it is not the P + 1 of a sum over the pairs (the conv-first composition sums P * HW per-pixel terms)."""
    x, w, b, dout, ou, s = i["x"], i["w"], i["b"], i["dout"], i["O_used"], i["scale"]
    P, C, HW, _ = x.shape
    mabs = x.abs().mean((2, 3))                                                    # [P, C]: mean_s |x|
    w2 = w.abs().reshape(w.shape[0], C)
    out = (HW + C + 3) * U * s * (b.abs()[None, :ou] + mabs @ w2[:ou].t())
    dx = (ou + 2) * U * (s / HW) * (dout.abs() @ w2[:ou])                          # [P, C]
    dw = torch.zeros_like(w2)
    dw[:ou] = (P + HW + 3) * U * s * (dout.abs().t() @ mabs)
    db = torch.zeros_like(b)
    db[:ou] = (dbias_ops or (P + 1)) * U * s * dout.abs().sum(0)
    return dict(out=SAFETY * out, dx=SAFETY * dx[:, :, None, None].expand(P, C, HW, 1), dw=SAFETY * dw.reshape(w.shape), dbias=SAFETY * db)


def tail_check(name, got, i, ref64=None, dbias_ops=None):
    """assert |got - fp64| <= bound element-wise for out, dx, dw, dbias; prints the worst used share of each bound."""
    ref64 = ref64 or tail_composed(i, torch.float64)
    bounds = tail_bounds(i, dbias_ops)
    for k in ("out", "dx", "dw", "dbias"):
        g, r, bd = got[k].detach().double().cpu().reshape(ref64[k].shape), ref64[k], bounds[k]
        assert torch.isfinite(g).all(), "%s %s: non-finite" % (name, k)
        err = (g - r).abs()
        used = float((err / bd.clamp(min=1e-300)).max())
        print("%s %-5s max err %.3g, worst share of the derived bound %.3f" % (name, k, float(err.max()), used))
        assert bool((err <= bd).all()), "%s %s: error %.3g exceeds the derived bound (%.3f of it)" % (name, k, float(err.max()), used)


# ------------------------------------------------------------------------------------------------------------ the whole network
NET_SHAPE = (2, 6, 64, 96)
DEC_FEATURE = (2, 512, 2, 3)
DECODER_KEYS = ["net.%d.%s" % (i, p) for i in range(4) for p in ("weight", "bias")]
DECODER_SHAPES = {"net.0.weight": (256, 512, 1, 1), "net.0.bias": (256,), "net.1.weight": (256, 256, 3, 3), "net.1.bias": (256,),
                  "net.2.weight": (256, 256, 3, 3), "net.2.bias": (256,), "net.3.weight": (12, 256, 1, 1), "net.3.bias": (12,)}


def grad_stride(numel):
    """sampling stride of a gradient's golden summary: every 53rd element of the small tensors, every 509th of the 3x3 weights"""
    return 53 if numel < 20000 else 509


def _bn_keys(p, c, sd):
    sd[p + ".weight"], sd[p + ".bias"] = torch.empty(c), torch.empty(c)
    sd[p + ".running_mean"], sd[p + ".running_var"] = torch.zeros(c), torch.ones(c)
    sd[p + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)


def encoder_state(tag="poseresnet:enc"):
    """State dict of ResnetEncoder(18, False, num_input_images=2) in torchvision's key order, detgen-filled."""
    sd = {"encoder.conv1.weight": torch.empty(64, 6, 7, 7)}
    _bn_keys("encoder.bn1", 64, sd)
    c_in = 64
    for li, c in enumerate((64, 128, 256, 512), start=1):
        for bi in range(2):
            p = "encoder.layer%d.%d" % (li, bi)
            sd[p + ".conv1.weight"] = torch.empty(c, c_in, 3, 3)
            _bn_keys(p + ".bn1", c, sd)
            sd[p + ".conv2.weight"] = torch.empty(c, c, 3, 3)
            _bn_keys(p + ".bn2", c, sd)
            if bi == 0 and li > 1:
                sd[p + ".downsample.0.weight"] = torch.empty(c, c_in, 1, 1)
                _bn_keys(p + ".downsample.1", c, sd)
            c_in = c
    sd["encoder.fc.weight"], sd["encoder.fc.bias"] = torch.empty(1000, 512), torch.empty(1000)
    return detgen.fill_state_dict(sd, tag)


def decoder_state(tag="poseresnet:dec"):
    return detgen.fill_state_dict({k: torch.empty(DECODER_SHAPES[k]) for k in DECODER_KEYS}, tag)


def net_input():
    b, c, h, w = NET_SHAPE
    return torch.cat([detgen.uniform((b, 3, h, w), "poseresnet:x%d" % i) for i in range(c // 3)], 1)      # images in [0, 1), as monodepth2 feeds


def decoder_feature():
    """A [2, 512, 2, 3] feature for the decoder alone: non-negative with exact zeros, as layer4's ReLU leaves it."""
    return torch.clamp(detgen.uniform(DEC_FEATURE, "poseresnet:feat", -0.5, 1.5), min=0.0)


def out_weights():
    b = NET_SHAPE[0]
    return detgen.uniform((b, 1, 1, 3), "poseresnet:ga", -1, 1), detgen.uniform((b, 1, 1, 3), "poseresnet:gt", -1, 1)


def pose_decoder_forward(sd, feat, num_frames_to_predict_for=2):
    """reference networks/pose_decoder.py:35-54 with one input feature -> (axisangle, translation), each [B, nf, 1, 3]"""
    out = F.relu(F.conv2d(feat, sd["net.0.weight"], sd["net.0.bias"]))
    out = F.relu(F.conv2d(out, sd["net.1.weight"], sd["net.1.bias"], 1, 1))
    out = F.relu(F.conv2d(out, sd["net.2.weight"], sd["net.2.bias"], 1, 1))
    out = F.conv2d(out, sd["net.3.weight"], sd["net.3.bias"])
    out = 0.01 * out.mean(3).mean(2).view(-1, num_frames_to_predict_for, 1, 6)
    return out[..., :3], out[..., 3:]


def first_transform_loss(aa, tr, dtype):
    """what monodepth2's trainer reads -- the FIRST predicted transform -- under the fixed output weights"""
    ga, gt = out_weights()
    return (aa[:, :1] * ga.to(dtype)).sum() + (tr[:, :1] * gt.to(dtype)).sum()


def _leaf(v, dtype):
    if not torch.is_floating_point(v):
        return v.clone()
    return v.to(dtype).clone().requires_grad_()


@functools.lru_cache(maxsize=None)
def decoder_reference(dtype):
    """the decoder alone on decoder_feature(): (axisangle, translation, {key: gradient})"""
    sd = {k: _leaf(v, dtype) for k, v in decoder_state().items()}
    aa, tr = pose_decoder_forward(sd, decoder_feature().to(dtype))
    first_transform_loss(aa, tr, dtype).backward()
    return aa.detach(), tr.detach(), {k: v.grad for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def net_reference(dtype, training=True):
    """encoder (train-mode BatchNorm: statistics over the batch) + decoder on net_input():
    (axisangle, translation, last feature, {encoder key: gradient}, {decoder key: gradient})"""
    esd = {k: (_leaf(v, dtype) if "running" not in k else v.to(dtype).clone()) for k, v in encoder_state().items()}
    dsd = {k: _leaf(v, dtype) for k, v in decoder_state().items()}
    feat = nets_res.resnet_encoder(esd, net_input().to(dtype), 18, training)[-1]
    aa, tr = pose_decoder_forward(dsd, feat)
    first_transform_loss(aa, tr, dtype).backward()
    eg = {k: v.grad for k, v in esd.items() if torch.is_floating_point(v) and v.requires_grad and ".fc." not in k}
    return aa.detach(), tr.detach(), feat.detach(), eg, {k: v.grad for k, v in dsd.items()}
