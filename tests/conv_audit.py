"""In-situ audit of every convolution call of a network's forward + backward against fp64 (a plain module, not a fixture file).

`audit(monkeypatch, net)` wraps engine.conv_forward / conv_dgrad / conv_wgrad (the block helpers look them up as module globals)
and, for every call the network makes on the data it actually produced:
  1. materialises what the call reads, as its operand descriptors define it (engine._fill_operand: a nearest x2 up-shift for `up`
     pieces, the pending BatchNorm scale / shift + ReLU for affine pieces, then the virtual concat), in fp64, together with the
     magnitudes |operand| the error bound needs; snapshots an output the call accumulates into;
  2. runs the call and synchronises;
  3. records layer name, pass, geometry, pieces and dn_last_kernel();
  4. evaluates the call's contract in fp64 (tap gather + matmul: the same code on the CPU or the GPU) and, with the same code on
     |operands| and |weights|, A = the per-element sum of |terms|;
  5. checks |got - ref| <= c * u * A + tiny on every checked element (u = 2^-24, c per kernel family and pass: bound()) and a
     relative L2 <= REL_L2.
Fused epilogues are checked against fp64 sums of the kernel's OWN output (or input), so that the reduction is tested apart from the
convolution's rounding: the forward's BatchNorm partial sums and their finalize (mean, invstd, scale / shift, running statistics --
folded into the launch or not), the input gradient's BatchNorm-backward sums (partial rows, and the folded d(gamma), d(beta)), the
bias gradient the weight-gradient call produces, and a disparity head's reciprocal (within 1 ulp of 1 / its own disparity).

Any network (or several, run in one step: `audit(monkeypatch, net_a, net_b)`): calls are named by their module's name in
named_modules(), the hot set is every nn.Conv2d / nn.ConvTranspose2d of the nets but the caller's exclusions, and a layer owes an
input-gradient call exactly when one of its input pieces needs a gradient.  Reflection-padded layers (ConvLayer(reflect_pad=p)) are
referenced over the reflected operand: the forward and weight gradient read the materialised input reflect-padded by p, the input
gradient folds the padded border back (the adjoint of the reflection).  The fused DORN head (engine.block_ord_head) is checked as a
whole: probabilities and decoded labels against the fp64 module sequence, and, through the closure it pushes on the tape, d(x),
d(W), d(b) against fp64.

Sampling: forward and input gradient reference the first, middle and last image in full (every border, every tile column, the
blocks of the last round); the weight gradient reduces over all N images for SAMPLED_CIN input channels x all output channels x all
taps.
"""
import contextlib
import inspect
import math
import os

import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # unit round-off of fp32
TINY = 2.0 ** -100             # absolute floor: far below any value these layers produce, far above fp64 round-off of zero
REL_L2 = 5e-6                  # the suite's convention for an fp32 result against fp64 (tests/test_gpu_f32x3_fp64.py)
SAMPLED_CIN = 8
# the relative L2 criterion is taken against max(|ref|, |A| / COND_MAX): where the exact result cancels by more than COND_MAX (a
# weight gradient in front of a BatchNorm, whose dy has zero mean per channel, reduced against all-positive ReLU / pool outputs:
# |ref| ~ |A| / 200 measured), fp32's own rounding of the terms, <= u |A|, is no longer small against |ref| and the per-element
# bound alone decides
COND_MAX = 100.0

# ------------------------------------------------------------------------------------------------------------- the bound
# c of |got - ref| <= c * u * A.  A sums |terms| of the exact convolution, so an fp32 dot product of K terms in ANY order stays below
# (K - 1) * u * A; the constants below are far tighter, and they have to be: dropping one of K = 576 terms moves a result by about
# A / 576 = 2.9e4 * u * A, a wrong tap or channel by as much, so every c here stays below 2^24 / K by orders of magnitude
# (tests/test_conv_audit_host.py proves the rejections at each family's K).  Calibrated on the f32 compute mode at the NYU and KITTI
# training / validation shapes (tests/test_gpu_nyu_shapes.py prints the worst err / (u A) per family), f32x3 held to the same values.
#
# direct kernels (implicit GEMM, lds3 / lds3k, stem, thin, heads): blocked fp32 FMA chains.  The round-offs of a chain of length L
# grow like sqrt(L) u A (independent errors on partial sums <= A); the longest sequential chain is one K slice of 9 x 128 terms:
# sqrt(1152) = 34 -> 32 (measured worst: 7.3 in f32).
C_DIRECT = 32
# Winograd F(2x2, 3x3) forward / input gradient: the products are formed on TRANSFORMED tiles.  The input transform B^T d B sums 4
# (= 2 x 2) inputs per transformed element with coefficients +-1, the filter transform G g G^T sums 9/4 of the weights' magnitude,
# the output transform A^T m A sums 9 products (3 x 3 ones): 4 * 9/4 * 9 = 81 as a worst-case growth of the transformed terms over
# the direct A, but the transformed chains are only K = Cin long and their errors are independent: sqrt(81) * sqrt(1152) / 4 ~ 77
# -> 64 (measured worst: 4.2 in f32, 7.7 in f32x3).
C_WINO = 64
# Weight gradients reduce over P = N * OH * OW pixels (N * IH * IW for the transposed convolution) by trees: a sequential run per
# thread, then wave, block and split partials merged pairwise.  Each level of a pairwise tree adds at most u * A; a run of L adds
# sqrt(L) u A in the independent-error model: with runs of <= 2^10 pixels, 32 + log2(P) bounds it; x 2 for the Winograd
# weight-gradient kernels, whose products are formed on 4 x 4 transformed tiles (measured worst: 9.5).
C_WGRAD_RUN = 32.0
C_WINO_WGRAD_GROWTH = 2.0
# fused reductions over the kernel's own output (BatchNorm partials: 128-pixel tiles summed sequentially, then merged in fp64 by
# the finalize; the bias gradient's two-stage column sums): a 128-long fp32 chain + one rounding of the summed values.
C_SUM = 130.0


def family(kernel):
    if kernel.startswith("dn::ord_head"):
        return "ord_head"
    if kernel.startswith("dn::wino_wgrad"):
        return "wino_wgrad"
    if kernel.startswith("dn::wino_conv"):
        return "wino"
    return "direct"


def bound(kernel, pas, P=1):
    """c for a call of `kernel` in pass `pas` ('fwd' / 'dgrad' / 'wgrad') reducing over P pixels (wgrad)."""
    fam = family(kernel)
    if pas == "wgrad":
        c = C_WGRAD_RUN + math.log2(max(P, 2))
        return c * C_WINO_WGRAD_GROWTH if fam == "wino_wgrad" else c
    return C_WINO if fam == "wino" else C_DIRECT


def compare(got, ref, A, c, act_slope=None, act_ulps=0.0, act_abs=None):
    """(ok, max err / (u A), relative L2, number of elements over the bound).  `act_slope` (per element) scales the bound of a
    pre-activation error through the activation; `act_ulps` allows that many ulps of |ref| for the activation's own evaluation;
    `act_abs` (per element, in units of u) an absolute error of that evaluation that is not relative to |ref|."""
    got = got.double()
    err = (got - ref).abs()
    allow = c * U * A
    if act_slope is not None:
        allow = allow * act_slope
    allow = allow + act_ulps * U * ref.abs() + TINY
    if act_abs is not None:
        allow = allow + U * act_abs
    over = int((err > allow).sum()) + int((~torch.isfinite(got)).sum())
    scale = U * (A * (act_slope if act_slope is not None else 1.0)) + TINY
    if act_abs is not None:
        scale = scale + U * (act_abs + act_ulps * ref.abs()) / c
    worst = float((err / scale).max()) if err.numel() else 0.0
    rel = float(err.norm() / (max(float(ref.norm()), float(A.norm()) / COND_MAX) + 1e-300)) if err.numel() else 0.0
    return over == 0 and rel <= REL_L2, worst, rel, over


# ------------------------------------------------------------------------------------------------------ fp64 reference
def nhwc_view(act):
    """The [N, H, W, C] logical view of an Act (any strides, e.g. a planar user image read through operand strides)."""
    return torch.as_strided(act.t, (act.N, act.H, act.W, act.C), act.strides, act.t.storage_offset())


def materialise(act, up=False, scale=None, shift=None, images=None, channels=None, relu=True):
    """One operand as its descriptor defines it: (value, magnitude) fp64 [n, H', W', c] for the selected images / channels.
    The magnitude is what the operand's own fp32 evaluation may be off by, in units of u: |x * scale| + |shift| where the pending
    affine + ReLU keeps (or nearly keeps) the value, else 0."""
    x = nhwc_view(act)
    if images is not None:
        x = x[images]
    if channels is not None:
        x = x[..., channels]
    x = x.double()
    if scale is not None:
        sc, sh = scale.double(), shift.double()
        if channels is not None:
            sc, sh = sc[channels], sh[channels]
        xs = x * sc
        pre = xs + sh
        mag = xs.abs() + sh.abs()
        if relu:
            val = pre.clamp_min(0)
            mag = torch.where(pre > -2.0 ** -20 * mag, mag, torch.zeros_like(mag))
        else:
            val = pre
    else:
        val, mag = x, x.abs()
    if up:
        val = val.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        mag = mag.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return val, mag


def _gather(x, r0, s0, stride, OH, OW):
    """x[:, r0 + i * stride, s0 + j * stride] for i < OH, j < OW, zero outside x (r0, s0 may be negative)."""
    n, H, W, C = x.shape
    lo_h, lo_w = max(0, -r0), max(0, -s0)
    hi_h = max(0, r0 + (OH - 1) * stride - (H - 1))
    hi_w = max(0, s0 + (OW - 1) * stride - (W - 1))
    if lo_h or lo_w or hi_h or hi_w:
        x = F.pad(x, (0, 0, lo_w, hi_w, lo_h, hi_h))
    r0 += lo_h
    s0 += lo_w
    return x[:, r0:r0 + (OH - 1) * stride + 1:stride, s0:s0 + (OW - 1) * stride + 1:stride]


def conv_nhwc(x, w, stride, pad, dil, OH, OW):
    """y[n, oh, ow, co] = sum_{ci, r, s} x[n, oh * stride - pad + r * dil, ow * stride - pad + s * dil, ci] w[co, ci, r, s]."""
    n = x.shape[0]
    Co, Ci, R, S = w.shape
    y = torch.zeros((n * OH * OW, Co), dtype=x.dtype, device=x.device)
    for r in range(R):
        for s in range(S):
            xs = _gather(x, r * dil - pad, s * dil - pad, stride, OH, OW).reshape(-1, Ci)
            y += xs @ w[:, :, r, s].t()
    return y.reshape(n, OH, OW, Co)


def convT_nhwc(x, w, stride, pad, OH, OW):
    """Transposed convolution, w [Cin, Cout, R, S]: y[n, ih * stride - pad + r, ...] += x[n, ih, ...] w[ci, co, r, s] -- a stride-1
    convolution of the zero-inserted input with the flipped, transposed filter."""
    n, H, W, Ci = x.shape
    R, S = w.shape[2], w.shape[3]
    z = torch.zeros((n, (H - 1) * stride + 1, (W - 1) * stride + 1, Ci), dtype=x.dtype, device=x.device)
    z[:, ::stride, ::stride] = x
    return conv_nhwc(z, w.flip(2, 3).transpose(0, 1), 1, R - 1 - pad, 1, OH, OW)


def _reflect_index(n, p, device=None):
    """Source row of each of the n + 2p rows of nn.ReflectionPad2d(p) over n rows: -i before row 0, 2(n-1) - i after row n-1."""
    i = torch.arange(-p, n + p, device=device)
    return torch.where(i < 0, -i, torch.where(i > n - 1, 2 * (n - 1) - i, i))


def reflect_pad(x, p):
    """x [n, H, W, C] reflection-padded by p on each side of H and W (the border row / column itself is not repeated)."""
    return x[:, _reflect_index(x.shape[1], p, x.device)][:, :, _reflect_index(x.shape[2], p, x.device)]


def reflect_fold(g, p):
    """Adjoint of reflect_pad: g [n, H + 2p, W + 2p, C] -> [n, H, W, C], every padded row / column added to the one it copies."""
    n, GH, GW, C = g.shape
    H, W = GH - 2 * p, GW - 2 * p
    rows = torch.zeros((n, H, GW, C), dtype=g.dtype, device=g.device).index_add_(1, _reflect_index(H, p, g.device), g)
    return torch.zeros((n, H, W, C), dtype=g.dtype, device=g.device).index_add_(2, _reflect_index(W, p, g.device), rows)


def fwd_ref(geo, X, W, bias):
    """Pre-activation forward of one call on a materialised input X [n, IH, IW, Cin] (reflection-padded first when geo["reflect"]:
    then geo["pad"] is the reflection's width and the convolution itself has none)."""
    pad = geo["pad"]
    if geo.get("reflect"):
        X, pad = reflect_pad(X, pad), 0
    if geo["transposed"]:
        y = convT_nhwc(X, W, geo["stride"], pad, geo["OH"], geo["OW"])
    else:
        y = conv_nhwc(X, W, geo["stride"], pad, geo["dil"], geo["OH"], geo["OW"])
    return y + bias if bias is not None else y


def dgrad_ref(geo, dY, W):
    """Gradient w.r.t. the (materialised, concatenated) forward input [n, IH, IW, Cin] of one call (through the reflection when
    geo["reflect"]: the gradient of the padded operand, its border folded back)."""
    if geo["transposed"]:
        return conv_nhwc(dY, W, geo["stride"], geo["pad"], 1, geo["IH"], geo["IW"])
    assert geo["dil"] == 1
    if geo.get("reflect"):
        p = geo["pad"]
        return reflect_fold(convT_nhwc(dY, W, geo["stride"], 0, geo["IH"] + 2 * p, geo["IW"] + 2 * p), p)
    return convT_nhwc(dY, W, geo["stride"], geo["pad"], geo["IH"], geo["IW"])


def wgrad_ref(geo, X, dY):
    """Weight gradient (framework layout) restricted to the input channels X holds: conv [Cout, c, R, S], convT [c, Cout, R, S]."""
    R, S, st, pad = geo["R"], geo["S"], geo["stride"], geo["pad"]
    if geo.get("reflect"):
        X, pad = reflect_pad(X, pad), 0
    c, Co = X.shape[-1], dY.shape[-1]
    if geo["transposed"]:
        out = torch.zeros((c, Co, R, S), dtype=X.dtype, device=X.device)
        xm = X.reshape(-1, c).t()
        for r in range(R):
            for s in range(S):
                out[:, :, r, s] = xm @ _gather(dY, r - pad, s - pad, st, geo["IH"], geo["IW"]).reshape(-1, Co)
        return out
    out = torch.zeros((Co, c, R, S), dtype=X.dtype, device=X.device)
    dm = dY.reshape(-1, Co).t()
    for r in range(R):
        for s in range(S):
            out[:, :, r, s] = dm @ _gather(X, r * geo["dil"] - pad, s * geo["dil"] - pad, st, geo["OH"], geo["OW"]).reshape(-1, c)
    return out


def fold_up(g):
    """Gradient of a nearest x2 up-shift: sum over each 2 x 2 block."""
    n, H, W, C = g.shape
    return g.reshape(n, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))


def activation(z, act, p0, p1):
    """(value, slope bound, ulps of |value|, absolute term in units of u) of the epilogue activation on fp64 pre-activations z."""
    from supervised_dispnet_amd._lib import ACT_ELU, ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID_AFFINE
    if act == ACT_NONE:
        return z, None, 0.0, None
    if act == ACT_RELU:
        return z.clamp_min(0), None, 0.0, None
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, z * p0), None, 2.0, None
    if act == ACT_SIGMOID_AFFINE:
        s = torch.sigmoid(z)
        # error of z propagates with slope p0 * s (1 - s); the activation's own exp / divide / FMA: a few ulps of the result
        return p0 * s + p1, (p0 * s * (1 - s)).clamp_min(2.0 ** -30), 8.0, None
    if act == ACT_ELU:
        # expf(z) - 1 for z <= 0 (alpha 1, the kernels' form): slope exp(z) <= 1; expf is within 2 ulps of exp(z) (4 u exp(z)
        # absolute) and the subtraction of 1 cancels, so that error is absolute, not relative to the result; + 1 ulp of the result
        e = torch.exp(z.clamp_max(0))
        return torch.where(z > 0, z, e - 1), torch.where(z > 0, torch.ones_like(z), e), 1.0, torch.where(z > 0, torch.zeros_like(z), 4 * e)
    raise NotImplementedError("activation %d" % act)


def sample_images(N):
    return sorted({0, N // 2, N - 1})


def host_threads():
    """torch CPU threads for host-side references: OMP_NUM_THREADS when set, never more than 16."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        n = 16
    return max(1, min(16, n))


@contextlib.contextmanager
def capped_threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(min(prev, host_threads()))
    try:
        yield
    finally:
        torch.set_num_threads(prev)


# ------------------------------------------------------------------------------------------------------------ the audit
class Audit(object):
    def __init__(self, nets, exclude=(), wgrad_channels=SAMPLED_CIN):
        """`nets`: the networks one step runs; `exclude`: names of convolutions of theirs the step does not run through the three
        wrapped entry points (e.g. DORN's conv_ord under the fused head).  With several nets a name is prefixed by its net's class."""
        from supervised_dispnet_amd import _lib, engine
        self.engine, self.lib = engine, _lib.load()
        self.names = {}               # id(module) -> name
        hot = []
        for net in nets:
            prefix = type(net).__name__ + ":" if len(nets) > 1 else ""
            for n, m in net.named_modules():
                if id(m) in self.names:
                    continue
                self.names[id(m)] = prefix + n
                if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                    hot.append(prefix + n)
        unknown = set(exclude) - set(hot)
        if unknown:
            raise KeyError("conv_audit: excluded layers that are no convolution of the nets: %s" % sorted(unknown))
        self.hot = sorted(set(hot) - set(exclude))
        self.needs_dx = {}            # layer -> whether a forward call read an input piece that needs a gradient
        self.rows = []
        self.failures = []
        self.pending = []             # forward BatchNorm statistics to check once their finalize has run
        self.wgrad_channels = wgrad_channels

    # -- bookkeeping
    def _name(self, layer):
        return self.names.get(id(layer.m), "?%s" % type(layer.m).__name__)

    def _row(self, name, pas, kernel, what, ok, worst, rel, over, geo=None, pieces=None, c=None):
        row = {"layer": name, "pass": pas, "kernel": kernel, "what": what, "ok": ok, "worst": worst, "rel": rel, "over": over, "c": c,
               "geo": geo, "pieces": pieces}
        self.rows.append(row)
        if not ok:
            self.failures.append(row)

    @staticmethod
    def _geo(layer, N, IH, IW, OH, OW):
        return {"N": N, "IH": IH, "IW": IW, "OH": OH, "OW": OW, "R": layer.R, "S": layer.S, "stride": layer.stride, "pad": layer.pad,
                "dil": layer.dil, "transposed": layer.transposed, "reflect": layer.reflect, "Cin": layer.Cin, "Cout": layer.Cout}

    def _kernel(self):
        return self.lib.dn_last_kernel().decode(errors="replace")

    @staticmethod
    def _operands(pieces, images=None, channels=None):
        """Materialised fp64 concat of the pieces (value, magnitude); `channels` index the concatenated channel axis."""
        vals, mags, c0 = [], [], 0
        for p in pieces:
            a = p.act
            sel = None
            if channels is not None:
                sel = [c - c0 for c in channels if c0 <= c < c0 + a.C]
                c0 += a.C
                if not sel:
                    continue
            v, m = materialise(a, p.up, a.scale, a.shift, images=images, channels=sel)
            vals.append(v)
            mags.append(m)
        return torch.cat(vals, dim=-1), torch.cat(mags, dim=-1)

    # -- fused epilogue checks
    def flush(self):
        """Check forward BatchNorm statistics whose finalize (folded into the launch or a launch of its own) has run by now."""
        if not self.pending:
            return
        torch.cuda.synchronize()
        for p in self.pending:
            self._check_bn_stats(**p)
        self.pending = []

    def _check_bn_stats(self, name, kernel, y, bn, rm0, rv0, mean, invstd, scale, shift, folded):
        Cn = y.shape[-1]
        y64 = y.reshape(-1, Cn).double()
        n = y64.shape[0]
        m64 = y64.mean(0)
        d = y64 - m64
        var = (d * d).mean(0)
        # the partial sums are taken of the fp32 accumulator before the bias is added and the result rounded: the statistics of the
        # stored y differ from them by one rounding of y per element, plus the 128-row chains
        A_mean = y64.abs().mean(0)
        what = "bn_stats%s" % ("(folded)" if folded else "")
        e_mean = (mean.double() - m64).abs()
        ok_m = bool((e_mean <= C_SUM * U * A_mean + TINY).all())
        A_var = 2 * (y64.abs() * d.abs()).mean(0)
        tol_var = C_SUM * U * A_var + TINY
        ref_inv = 1.0 / torch.sqrt(var + bn.eps)
        # invstd = 1 / sqrt(var + eps): relative error half the variance's, plus the fp32 rounding of the result
        tol_inv = ref_inv * (0.5 * tol_var / (var + bn.eps) + 4 * U)
        e_inv = (invstd.double() - ref_inv).abs()
        ok_i = bool((e_inv <= tol_inv).all())
        g, b = bn.weight.detach().double(), bn.bias.detach().double()
        sc_ref = g * invstd.double()
        ok_s = bool(((scale.double() - sc_ref).abs() <= 2 * U * sc_ref.abs() + TINY).all())
        sh_ref = b - mean.double() * scale.double()
        ok_h = bool(((shift.double() - sh_ref).abs() <= 4 * U * (b.abs() + (mean.double() * scale.double()).abs()) + TINY).all())
        mom = bn.momentum if bn.momentum is not None else self.engine.BN_MOMENTUM
        rm_ref = (1 - mom) * rm0 + mom * m64
        ok_rm = bool(((bn.running_mean.double() - rm_ref).abs() <= mom * C_SUM * U * A_mean + 4 * U * ((1 - mom) * rm0.abs() + mom * m64.abs()) + TINY).all())
        unb = n / (n - 1.0)
        rv_ref = (1 - mom) * rv0 + mom * var * unb
        ok_rv = bool(((bn.running_var.double() - rv_ref).abs() <= mom * unb * tol_var + 4 * U * ((1 - mom) * rv0.abs() + mom * unb * var) + TINY).all())
        worst = max(float((e_mean / (U * A_mean + TINY)).max()), float((e_inv / (ref_inv * U)).max()))
        parts = {"mean": ok_m, "invstd": ok_i, "scale": ok_s, "shift": ok_h, "running_mean": ok_rm, "running_var": ok_rv}
        ok = all(parts.values())
        self._row(name, "fwd", kernel, what if ok else what + " bad:" + ",".join(k for k, v in parts.items() if not v), ok, worst, 0.0,
                  0 if ok else 1, c=C_SUM)

    def _check_partial_sum(self, name, kernel, partial, y, bias):
        """Sum over the partial rows' first component (sum of the pre-bias result) vs fp64 sum of the kernel's own y - bias."""
        Cn = y.shape[-1]
        y64 = y.reshape(-1, Cn).double()
        if bias is not None:
            y64 = y64 - bias.double()
        got = partial[..., 0].double().sum(0)
        ref = y64.sum(0)
        A = y64.abs().sum(0) + (bias.double().abs() * y64.shape[0] if bias is not None else 0)
        ok, worst, rel, over = compare(got, ref, A, C_SUM)
        self._row(name, "fwd", kernel, "bn_partial_sum", over == 0, worst, rel, over, c=C_SUM)

    def _check_dgrad_bn_sums(self, name, kernel, a, partial, final):
        """BatchNorm-backward sums the input-gradient epilogue took of its own output: (sum dz, sum dz * xhat) per channel,
        dz = grad * [y * scale + shift > 0], xhat = (y - mean) * invstd."""
        Cn = a.C
        g = a.grad.reshape(-1, Cn).double()
        y64 = a.t.reshape(-1, Cn).double()
        sc, sh = a.scale.double(), a.shift.double()
        pre = y64 * sc + sh                   # (y * scale is exact in fp64: the sign of the fused multiply-add the kernel evaluates)
        dz = torch.where(pre > 0, g, torch.zeros_like(g))
        xhat = (y64 - a.mean.double()) * a.invstd.double()
        # where y * scale + shift lies within two roundings of 0, an fp32 evaluation without the fused multiply-add may take the
        # other side of the ReLU: those elements may count either way
        amb = (pre.abs() <= 2 * U * ((y64 * sc).abs() + sh.abs())).double()
        ref0, ref1 = dz.sum(0), (dz * xhat).sum(0)
        A0 = dz.abs().sum(0) + (amb * g.abs()).sum(0) / (C_SUM * U)
        A1 = (dz.abs() * (y64.abs() + a.mean.double().abs()) * a.invstd.double()).sum(0) + (amb * (g * xhat).abs()).sum(0) / (C_SUM * U)
        got0 = partial[..., 0].double().sum(0)
        got1 = partial[..., 1].double().sum(0)
        res = [compare(got0, ref0, A0, C_SUM), compare(got1, ref1, A1, C_SUM)]
        if final is not None:
            dg, db = final
            res += [compare(db, ref0, A0, C_SUM), compare(dg, ref1, A1, C_SUM)]
        ok = all(r[3] == 0 for r in res)
        self._row(name, "dgrad", kernel, "bn_bwd_sums%s" % ("(folded)" if final is not None else ""), ok, max(r[1] for r in res),
                  max(r[2] for r in res), sum(r[3] for r in res), c=C_SUM)

    def _check_partial_sum_preact(self, name, kernel, partial, pieces, geo, Wt):
        """The partial rows of a layer with an epilogue activation (Disp_res_50's conv1: the statistics of a BatchNorm the
        reference computes from the pre-activation and discards) sum the pre-bias, pre-activation result, which the kernel does
        not store: against the fp64 convolution of all images, with the convolution's bound + the sum's."""
        ref = A = 0
        for i0 in range(0, geo["N"], 4):
            X, Xm = self._operands(pieces, images=list(range(i0, min(geo["N"], i0 + 4))))
            z = fwd_ref(geo, X, Wt, None)
            ref = ref + z.reshape(-1, z.shape[-1]).sum(0)
            A = A + fwd_ref(geo, Xm, Wt.abs(), None).reshape(-1, z.shape[-1]).sum(0)
        c = C_DIRECT + C_SUM
        ok, worst, rel, over = compare(partial[..., 0].double().sum(0), ref, A, c)
        self._row(name, "fwd", kernel, "bn_partial_sum(pre-act)", over == 0, worst, rel, over, c=c)

    # -- the three wrapped entry points
    def conv_forward(self, orig, *args, **kwargs):
        ba = inspect.signature(orig).bind(*args, **kwargs)
        ba.apply_defaults()
        A_ = ba.arguments
        from supervised_dispnet_amd._lib import ACT_NONE as ACT_NONE_
        layer, pieces, act, p0, p1 = A_["layer"], A_["pieces"], A_["act"], A_["p0"], A_["p1"]
        if A_["out_view"] is not None:
            raise NotImplementedError("conv_audit: out_view is not audited")
        self.flush()
        torch.cuda.synchronize()
        a0 = pieces[0].act
        N = a0.N
        IH, IW = a0.H * (2 if pieces[0].up else 1), a0.W * (2 if pieces[0].up else 1)
        OH, OW = A_["out_hw"] or layer.out_size(IH, IW)
        geo = self._geo(layer, N, IH, IW, OH, OW)
        imgs = sample_images(N)
        X, Xm = self._operands(pieces, images=imgs)
        bn = A_["bn_fold"][0] if A_["bn_fold"] is not None else None
        rm0 = bn.running_mean.detach().double().clone() if bn is not None else None
        rv0 = bn.running_var.detach().double().clone() if bn is not None else None
        recip = A_["recip"]
        y, partial, rows = orig(*args, **kwargs)
        torch.cuda.synchronize()
        kernel = self._kernel()
        name = self._name(layer)
        Wt = layer.m.weight.detach().double()
        b = layer.m.bias.detach().double() if layer.m.bias is not None else None
        z = fwd_ref(geo, X, Wt, b)
        Az = fwd_ref(geo, Xm, Wt.abs(), b.abs() if b is not None else None)
        ref, slope, ulps, absu = activation(z, act, p0, p1)
        c = bound(kernel, "fwd")
        ok, worst, rel, over = compare(y[imgs], ref, Az, c, slope, ulps, absu)
        self.needs_dx[name] = self.needs_dx.get(name, False) or any(p.act.needs_grad for p in pieces)
        self._row(name, "fwd", kernel, "y", ok, worst, rel, over, geo, [(p.act.C, p.up, p.act.scale is not None) for p in pieces], c)
        if partial is not None and act == ACT_NONE_:
            self._check_partial_sum(name, kernel, partial, y, layer.m.bias.detach() if layer.m.bias is not None else None)
        elif partial is not None:
            self._check_partial_sum_preact(name, kernel, partial, pieces, geo, Wt)
        if bn is not None:
            fold = A_["bn_fold"]
            self.pending.append({"name": name, "kernel": kernel, "y": y, "bn": bn, "rm0": rm0, "rv0": rv0, "mean": fold[1],
                                 "invstd": fold[2], "scale": fold[3], "shift": fold[4], "folded": fold[0] is True})
        if recip:
            r = recip[0].double()
            ref_r = 1.0 / y.double()
            ulp = torch.pow(2.0, torch.floor(torch.log2(ref_r.abs())) - 23)
            e = (r - ref_r).abs()
            over = int((e > ulp).sum())
            self._row(name, "fwd", kernel, "recip", over == 0, float((e / ulp).max()), 0.0, over, c=1.0)
        return y, partial, rows

    def conv_dgrad(self, orig, *args, **kwargs):
        ba = inspect.signature(orig).bind(*args, **kwargs)
        A_ = ba.arguments
        layer, dy, N, OH, OW, pieces, in_hw = (A_[k] for k in ("layer", "dy", "N", "OH", "OW", "pieces", "in_hw"))
        if not any(p.act.needs_grad for p in pieces):
            return orig(*args, **kwargs)
        self.flush()
        torch.cuda.synchronize()
        IH, IW = in_hw
        geo = self._geo(layer, N, IH, IW, OH, OW)
        imgs = sample_images(N)
        pre = []
        for p in pieces:
            a = p.act
            pre.append(a.grad[imgs].double().clone() if (a.needs_grad and a.grad is not None) else None)
        sums_before = [p.act.bn_sums for p in pieces]
        orig(*args, **kwargs)
        torch.cuda.synchronize()
        kernel = self._kernel()
        name = self._name(layer)
        Wt = layer.m.weight.detach().double()
        dY = dy[imgs].double()
        ref = dgrad_ref(geo, dY, Wt)
        Aref = dgrad_ref(geo, dY.abs(), Wt.abs())
        c = bound(kernel, "dgrad")
        c0 = 0
        res = []
        for p, before, sb in zip(pieces, pre, sums_before):
            a = p.act
            r, Ar = ref[..., c0:c0 + a.C], Aref[..., c0:c0 + a.C]
            c0 += a.C
            if not a.needs_grad:
                continue
            if p.up:
                r, Ar = fold_up(r), fold_up(Ar)
            got = a.grad[imgs].double()
            if before is not None:
                got = got - before
                Ar = Ar + before.abs()            # the accumulation's own rounding: one ulp of the sum
            res.append(compare(got, r, Ar, c))
            if a.bn_sums is not None and a.bn_sums is not sb:
                self._check_dgrad_bn_sums(name, kernel, a, a.bn_sums.partial, a.bn_sums.final)
        ok = all(x[0] for x in res)
        self._row(name, "dgrad", kernel, "dx", ok, max(x[1] for x in res), max(x[2] for x in res), sum(x[3] for x in res), geo,
                  [(p.act.C, p.up, p.act.scale is not None, p.act.grad is not None) for p in pieces], c)

    def conv_wgrad(self, orig, *args, **kwargs):
        ba = inspect.signature(orig).bind(*args, **kwargs)
        ba.apply_defaults()
        A_ = ba.arguments
        layer, pieces, dy, out_hw, out, sink, first = (A_[k] for k in ("layer", "pieces", "dy", "out_hw", "out", "sink", "first"))
        self.flush()
        torch.cuda.synchronize()
        a0 = pieces[0].act
        N = a0.N
        IH, IW = a0.H * (2 if pieces[0].up else 1), a0.W * (2 if pieces[0].up else 1)
        OH, OW = out_hw
        geo = self._geo(layer, N, IH, IW, OH, OW)
        cin = sum(p.act.C for p in pieces)
        chans = sorted(set(int(round(i * (cin - 1) / max(1, self.wgrad_channels - 1))) for i in range(self.wgrad_channels)))
        X, Xm = self._operands(pieces, channels=chans)
        dY = dy.double()
        dw = orig(*args, **kwargs)
        torch.cuda.synchronize()
        kernel = self._kernel()
        name = self._name(layer)
        ref = wgrad_ref(geo, X, dY)
        Aref = wgrad_ref(geo, Xm, dY.abs())
        got = dw[chans] if layer.transposed else dw[:, chans]
        P = N * (IH * IW if layer.transposed else OH * OW)
        c = bound(kernel, "wgrad", P)
        ok, worst, rel, over = compare(got, ref, Aref, c)
        self._row(name, "wgrad", kernel, "dw", ok, worst, rel, over, geo, [(p.act.C, p.up, p.act.scale is not None) for p in pieces], c)
        if first is not None and layer.m.bias is not None and sink is not None:
            db = sink.get(layer.m.bias)
            if db is None:
                db = sink.dest(layer.m.bias)
            if db is not None:
                d2 = dY.reshape(-1, dY.shape[-1])
                ok, worst, rel, over = compare(db, d2.sum(0), d2.abs().sum(0), C_SUM)
                self._row(name, "wgrad", "dn::colreduce_kernel", "db", ok, worst, rel, over, c=C_SUM)
        return dw

    # -- the fused DORN head
    def block_ord_head(self, orig, tape, sink, x, conv, mask):
        """Forward: probabilities and decoded labels of the sampled images against the fp64 module sequence (mask, 1 x 1 conv,
        clamp to [1e-8, 1e8], pair softmax); backward (the closure the block pushes on the tape, wrapped): d(x) of the sampled
        images, d(W) and d(b) over all N H W pixels."""
        self.flush()
        torch.cuda.synchronize()
        K = conv.out_channels // 2
        name = self.names.get(id(conv), "?ord_head")

        class _Tape(object):
            def push(_self, fn, out=None):
                tape.push(lambda: self._ord_head_bwd(fn, name, x, conv, mask, o, K, sink), out)

        o, d = orig(_Tape(), sink, x, conv, mask)
        torch.cuda.synchronize()
        imgs = sample_images(x.N)
        P, allow, _, _ = self._ord_head_ref(x, conv, mask, imgs)
        inexact = allow > TINY
        got = o.t[imgs].permute(0, 2, 3, 1)
        # c: the 16-term dot product + bias of a logit in fp32 in any order is within 16 u A of exact (C_DIRECT >= 16 covers the
        # worst case, not only the statistical one); the clamp is 1-Lipschitz; the pair softmax sigmoid(b - a) passes an error of
        # (a, b) on with slope P (1 - P); its exp and divide: a few ulps of P
        ok, worst, rel, over = compare(got, P[0], P[1], C_DIRECT, P[2], 8.0 * inexact.double())
        self._row(name, "fwd", "dn::ord_head_fwd_kernel", "P", ok, worst, rel, over, c=C_DIRECT)
        # decoded label = #{k: P_k > 0.5}: exact wherever no P of the pixel lies within its bound of 0.5
        dec_ref = (P[0] > 0.5).sum(-1)
        amb = (((P[0] - 0.5).abs() <= allow) & inexact).any(-1)
        bad = (d.t[imgs, 0].to(dec_ref.device) != dec_ref) & ~amb
        nbad = int(bad.sum())
        self._row(name, "fwd", "dn::ord_head_fwd_kernel", "decode(%d amb)" % int(amb.sum()), nbad == 0, 0.0, 0.0, nbad, c=0.0)
        return o, d

    def _ord_head_ref(self, x, conv, mask, imgs):
        """fp64 ((P, A of P's logits, slope), |P - ref| allowance, logits z, their A) of images `imgs`, NHWC / [..., 2K]."""
        xm = nhwc_view(x)[imgs].double()
        if mask is not None:
            xm = xm * mask[imgs].double()[:, None, None, :]
        Wt = conv.weight.detach().double().reshape(conv.out_channels, -1)
        b = conv.bias.detach().double()
        z = xm @ Wt.t() + b
        Az = xm.abs() @ Wt.abs().t() + b.abs()
        a_, b_ = z[..., 0::2].clamp(1e-8, 1e8), z[..., 1::2].clamp(1e-8, 1e8)
        P = torch.sigmoid(b_ - a_)
        # a logit further than its bound below 1e-8 is clamped exactly, whatever its error: it adds nothing to the error of b - a;
        # a pair clamped on both sides has b - a = 0 and P = 1 / (1 + exp(0)) = 0.5 exactly (allowance 0)
        live_a = z[..., 0::2] > 1e-8 - C_DIRECT * U * Az[..., 0::2]
        live_b = z[..., 1::2] > 1e-8 - C_DIRECT * U * Az[..., 1::2]
        A = Az[..., 0::2] * live_a + Az[..., 1::2] * live_b
        slope = (P * (1 - P)).clamp_min(2.0 ** -30)
        allow = (C_DIRECT * U * A * slope + 8.0 * U * P) * (live_a | live_b) + TINY
        return (P, A, slope), allow, z, Az

    def _ord_head_bwd(self, fn, name, x, conv, mask, o, K, sink):
        if o.grad is None:
            return fn()
        self.flush()
        torch.cuda.synchronize()
        N = x.N
        imgs = sample_images(N)
        G = o.grad.double()                                   # [N, K, H, W] planar
        before = x.grad[imgs].double().clone() if (x.needs_grad and x.grad is not None) else None
        fn()
        torch.cuda.synchronize()
        kern = "dn::ord_head_bwd_kernel"
        dW = dB = AW = AB = None
        dx_ref = dx_A = None
        for n in range(N):
            (P, _A, _s), allow, z, Az = self._ord_head_ref(x, conv, mask, [n])
            g = G[n:n + 1].permute(0, 2, 3, 1)                # [1, H, W, K]
            s = P * (1 - P)
            live_a = (z[..., 0::2] > 1e-8) & (z[..., 0::2] < 1e8)
            live_b = (z[..., 1::2] > 1e-8) & (z[..., 1::2] < 1e8)
            dz = torch.zeros_like(z)
            dz[..., 0::2] = -g * s * live_a
            dz[..., 1::2] = g * s * live_b
            # what the kernel's dz may be off by, in units of u: its recomputed P carries the forward's error (allow) into
            # s = P (1 - P) with slope |1 - 2P|, + a few ulps of its own products; a logit within its bound of the clamp's edge may
            # take either side of it (then the whole term)
            e = g.abs() * ((1 - 2 * P).abs() * allow / U + 4 * s)
            za, zb = z[..., 0::2], z[..., 1::2]
            tol_a, tol_b = C_DIRECT * U * Az[..., 0::2] + TINY, C_DIRECT * U * Az[..., 1::2] + TINY
            amb_a = ((za - 1e-8).abs() <= tol_a) | ((za - 1e8).abs() <= tol_a)
            amb_b = ((zb - 1e-8).abs() <= tol_b) | ((zb - 1e8).abs() <= tol_b)
            edz = torch.zeros_like(z)
            edz[..., 0::2] = e + amb_a * (g * s).abs() / U
            edz[..., 1::2] = e + amb_b * (g * s).abs() / U
            xm = nhwc_view(x)[n:n + 1].double()
            mk = mask[n].double() if mask is not None else None
            if mk is not None:
                xm = xm * mk
            dz2, edz2, xm2 = dz.reshape(-1, 2 * K), edz.reshape(-1, 2 * K), xm.reshape(-1, xm.shape[-1])
            Wt = conv.weight.detach().double().reshape(2 * K, -1)
            w_ = dz2.t() @ xm2
            aw = dz2.abs().t() @ xm2.abs() + (edz2.t() @ xm2.abs()) / (C_WGRAD_RUN + math.log2(N * x.H * x.W))
            b_, ab = dz2.sum(0), dz2.abs().sum(0) + edz2.sum(0) / (C_WGRAD_RUN + math.log2(N * x.H * x.W))
            dW, AW = (w_, aw) if dW is None else (dW + w_, AW + aw)
            dB, AB = (b_, ab) if dB is None else (dB + b_, AB + ab)
            if n in imgs:
                r = dz2 @ Wt
                ar = dz2.abs() @ Wt.abs() + (edz2 @ Wt.abs()) / C_DIRECT
                if mk is not None:
                    r, ar = r * mk, ar * mk.abs()
                dx_ref = r if dx_ref is None else torch.cat([dx_ref, r])
                dx_A = ar if dx_A is None else torch.cat([dx_A, ar])
        if x.needs_grad:
            got = x.grad[imgs].double().reshape(-1, x.C)
            if before is not None:
                got = got - before.reshape(-1, x.C)
                dx_A = dx_A + before.reshape(-1, x.C).abs()
            # dx: a 2K-term sum per element, c as for a direct kernel
            ok, worst, rel, over = compare(got, dx_ref, dx_A, C_DIRECT)
            self._row(name, "dgrad", kern, "head_dx", ok, worst, rel, over, c=C_DIRECT)
        P_ = N * x.H * x.W
        c = C_WGRAD_RUN + math.log2(max(P_, 2))
        dw = sink.get(conv.weight)
        dw = dw if dw is not None else sink.dest(conv.weight)
        db = sink.get(conv.bias)
        db = db if db is not None else sink.dest(conv.bias)
        ok, worst, rel, over = compare(dw.reshape(2 * K, -1), dW, AW, c)
        self._row(name, "wgrad", kern, "head_dw", ok, worst, rel, over, c=c)
        ok, worst, rel, over = compare(db, dB, AB, c)
        self._row(name, "wgrad", kern, "head_db", ok, worst, rel, over, c=c)

    # -- results
    def coverage(self, training):
        """Per pass, the hot layers whose calls were audited a wrong number of times: {} when every call was seen exactly once (a
        layer's input gradient only where one of its input pieces needs a gradient: not the stems, which read the images)."""
        counts = {}
        for r in self.rows:
            if r["what"] in ("y", "dx", "dw"):
                counts.setdefault(r["pass"], {}).setdefault(r["layer"], 0)
                counts[r["pass"]][r["layer"]] += 1
        bad = {}
        passes = ("fwd", "dgrad", "wgrad") if training else ("fwd",)
        for pas in passes:
            seen = counts.get(pas, {})
            for n in self.hot:
                want = 0 if (pas == "dgrad" and not self.needs_dx.get(n, True)) else 1
                if seen.get(n, 0) != want:
                    bad.setdefault(pas, {})[n] = seen.get(n, 0)
            for n in seen:
                if n not in self.hot:
                    bad.setdefault(pas, {})[n] = seen[n]
        return bad

    def kernels(self):
        return sorted({r["kernel"] for r in self.rows if r["what"] in ("y", "dx", "dw")})

    def table(self):
        lines = ["%-22s %-5s %-70s %-22s %10s %10s %s" % ("layer", "pass", "kernel", "check", "err/(uA)", "relL2", "c")]
        for r in self.rows:
            lines.append("%-22s %-5s %-70s %-22s %10.3g %10.3g %s%s" % (r["layer"], r["pass"], r["kernel"][:70], r["what"], r["worst"], r["rel"],
                                                                  "%.4g" % r["c"] if r["c"] is not None else "-", "" if r["ok"] else "   <-- FAIL"))
        return "\n".join(lines)

    def worst_by_family(self):
        out = {}
        for r in self.rows:
            if r["what"] in ("y", "dx", "dw", "P", "head_dx", "head_dw", "head_db"):
                k = (family(r["kernel"]), r["pass"])
                out[k] = max(out.get(k, 0.0), r["worst"])
        return out


def audit(monkeypatch, *nets, **kw):
    """Install the wrappers for the rest of the test (monkeypatch undoes them); returns the Audit collecting the rows.
    `exclude=(names...)`: convolutions of the nets that do not run through the wrapped entry points."""
    from supervised_dispnet_amd import engine
    a = Audit(nets, **kw)
    for fn in ("conv_forward", "conv_dgrad", "conv_wgrad", "block_ord_head"):
        orig = getattr(engine, fn)
        method = getattr(a, fn)
        monkeypatch.setattr(engine, fn, (lambda o, m: (lambda *args, **kwargs: m(o, *args, **kwargs)))(orig, method))
    return a
