"""Host checks of tests/conv_audit.py, the fp64 audit the GPU tests put around every convolution call (no GPU needed).

  * the audit's fp64 reference of each operand form -- a concat of 2 or 3 pieces, an up-shifted 1-channel piece, a BatchNorm-pending
    affine piece, the 4 x 4 stride-2 transposed convolution, the 3 x 3 convolution -- equals torch fp64 (F.conv2d /
    F.conv_transpose2d / autograd) applied to the independently materialised input, for the forward, the input gradient (folded
    through the up-shift) and the weight gradient;
  * sensitivity: at the K of every layer family Disp_vgg_BN's census shows, the bound accepts an honest fp32 result and rejects it
    after one tap shifted, one input channel dropped, one concat piece's channels permuted, the last output row zeroed -- and, for
    the weight gradient, one 1/splits share of the pixels dropped.  This is the evidence that the GPU audit would fail on a subtly
    wrong kernel.
  * the same for the forms and families of Disp_res_50, monodepth2 (ResnetEncoder(50) + the reflection-padded DepthDecoder) and
    PoseExpNet (tests/test_gpu_zoo_shapes.py): the 1 x 1 (stride 1 and 2), 7 x 7 / 2 and 5 x 5 / 2 convolutions, the stem over three
    planar frames, the 3 x 3 / 2 transposed convolution with output padding, reflection padding alone and behind an up-shifted piece
    + a skip; a reflection-padded family must also reject its border replicated instead of reflected.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_audit as CA  # noqa: E402
from supervised_dispnet_amd import engine  # noqa: E402


def _piece(g, N, H, W, C, up=False, affine=False, planar=False):
    """A CPU Act: post-ReLU-like values, or pre-BatchNorm values with a pending (scale, shift) + ReLU; `planar`: an [N, C, H, W]
    image read through operand strides (Act.from_nchw_image, as the stems read the user's frames)."""
    if planar:
        return engine.Piece(engine.Act.from_nchw_image(torch.rand(N, C, H, W, generator=g) * 2.0 - 1.0), up=up)
    if affine:
        t = torch.randn(N, H, W, C, generator=g) * 3.0 + 0.5
        a = engine.Act(t, N, H, W, C)
        a.scale = torch.rand(C, generator=g) * 0.5 + 0.2
        a.shift = torch.randn(C, generator=g) * 0.2
    else:
        a = engine.Act(torch.rand(N, H, W, C, generator=g) * 2.0, N, H, W, C)
    return engine.Piece(a, up=up)


def _logical(p, dtype=torch.float64):
    """The piece's logical value [N, C, h, w] (what Act.grad is the gradient of), materialised independently of the audit."""
    x = CA.nhwc_view(p.act).to(dtype)
    if p.act.scale is not None:
        x = torch.relu(x * p.act.scale.to(dtype) + p.act.shift.to(dtype))
    return x.permute(0, 3, 1, 2)


def _input(leaves, pieces):
    xs = [F.interpolate(x, scale_factor=2, mode="nearest") if p.up else x for x, p in zip(leaves, pieces)]
    return torch.cat(xs, dim=1)


# geometry of a form / family: (R, stride, pad, output padding, reflection); the default is the 3 x 3 convolution or the 4 x 4
# stride-2 transposed one
def _gm(entry):
    if len(entry) > 4:
        return entry[4]
    return (4, 2, 1, 0, False) if entry[3] else (3, 1, 1, 0, False)


def _geo_of(gm, transposed, N, IH, IW, Cin, Cout):
    R, st, pad, op, refl = gm
    if transposed:
        OH, OW = (IH - 1) * st - 2 * pad + R + op, (IW - 1) * st - 2 * pad + R + op
    else:
        OH, OW = (IH + 2 * pad - R) // st + 1, (IW + 2 * pad - R) // st + 1
    return {"N": N, "IH": IH, "IW": IW, "OH": OH, "OW": OW, "R": R, "S": R, "stride": st, "pad": pad, "dil": 1, "transposed": transposed,
            "reflect": refl, "Cin": Cin, "Cout": Cout}


def _geo(transposed, N, IH, IW, Cin, Cout):
    if transposed:
        return {"N": N, "IH": IH, "IW": IW, "OH": 2 * IH, "OW": 2 * IW, "R": 4, "S": 4, "stride": 2, "pad": 1, "dil": 1, "transposed": True,
                "Cin": Cin, "Cout": Cout}
    return {"N": N, "IH": IH, "IW": IW, "OH": IH, "OW": IW, "R": 3, "S": 3, "stride": 1, "pad": 1, "dil": 1, "transposed": False,
            "Cin": Cin, "Cout": Cout}


def _weights(g, transposed, cin, cout, dtype=torch.float64, R=None):
    R = R or (4 if transposed else 3)
    shape = (cin, cout, R, R) if transposed else (cout, cin, R, R)
    rf = shape[2] * shape[3]
    b = (6.0 / ((cin + cout) * rf)) ** 0.5
    return ((torch.rand(shape, generator=g) * 2 - 1) * b).to(dtype), ((torch.rand(cout, generator=g) * 2 - 1) * 0.05).to(dtype)


def _torch_conv(x, w, b, transposed, gm=None, pad_mode="reflect"):
    if gm is None:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1) if transposed else F.conv2d(x, w, b, padding=1)
    R, st, pad, op, refl = gm
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=st, padding=pad, output_padding=op)
    if refl:
        return F.conv2d(F.pad(x, (pad,) * 4, mode=pad_mode), w, b, stride=st)
    return F.conv2d(x, w, b, stride=st, padding=pad)


# (id, piece list [(channels, up, affine)], Cout, transposed)
FORMS = [("conv3x3_affine", [(24, False, True)], 16, False),
         ("concat2", [(16, False, False), (24, False, True)], 8, False),
         ("concat3_with_up1", [(8, False, False), (16, False, False), (1, True, False)], 8, False),
         ("up1_only", [(1, True, False)], 4, False),
         ("convT4x4s2_affine", [(12, False, True)], 8, True),
         # ... and the forms of the other networks: DepthDecoder's reflection-padded 3 x 3 (alone; an up-shifted piece + a skip piece),
         # ResNet's 1 x 1 stride-2 downsample, PoseExpNet's 7 x 7 / 2 stem over three planar frames and its 5 x 5 / 2, Disp_res_50's
         # 3 x 3 / 2 transposed convolution with output padding
         ("reflect3x3", [(12, False, False)], 8, False, (3, 1, 1, 0, True)),
         ("reflect3x3_up_skip", [(8, True, False), (12, False, False)], 8, False, (3, 1, 1, 0, True)),
         ("conv1x1s2_affine", [(16, False, True)], 8, False, (1, 2, 0, 0, False)),
         ("stem7x7s2_3planar", [(3, False, False, True), (3, False, False, True), (3, False, False, True)], 8, False, (7, 2, 3, 0, False)),
         ("conv5x5s2", [(12, False, False)], 8, False, (5, 2, 2, 0, False)),
         ("convT3x3s2_outpad", [(12, False, False)], 8, True, (3, 2, 1, 1, False))]


def _pieces(g, spec, N, H, W):
    return [_piece(g, N, H // 2 if sp[1] else H, W // 2 if sp[1] else W, *sp) for sp in spec]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_reference_matches_torch_fp64_on_the_materialised_input(form):
    spec, cout, tr, gm = form[1], form[2], form[3], _gm(form)
    g = torch.Generator().manual_seed(3)
    N, H, W = 3, 6, 10
    pieces = _pieces(g, spec, N, H, W)
    cin = sum(sp[0] for sp in spec)
    w, b = _weights(g, tr, cin, cout, R=gm[0])
    geo = _geo_of(gm, tr, N, H, W, cin, cout)
    leaves = [_logical(p).clone().requires_grad_(True) for p in pieces]
    wl = w.clone().requires_grad_(True)
    y = _torch_conv(_input(leaves, pieces), wl, b, tr, gm)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    # forward on the audit's materialisation (all images, all channels)
    X, Xm = CA.Audit._operands(pieces, images=list(range(N)))
    ref = CA.fwd_ref(geo, X, w, b)
    assert torch.allclose(ref, y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert bool((Xm >= X.abs() - 1e-12).all())                      # magnitudes bound the operands
    # input gradient, split per piece and folded through the up-shift
    dY = dy.permute(0, 2, 3, 1)
    dx = CA.dgrad_ref(geo, dY, w)
    c0 = 0
    for p, leaf in zip(pieces, leaves):
        part = dx[..., c0:c0 + p.C]
        c0 += p.C
        if p.up:
            part = CA.fold_up(part)
        assert torch.allclose(part, leaf.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    # weight gradient at sampled input channels of the concat
    chans = [0, cin // 2, cin - 1]
    Xc, _ = CA.Audit._operands(pieces, channels=chans)
    dw = CA.wgrad_ref(geo, Xc, dY)
    want = wl.grad[chans] if tr else wl.grad[:, chans]
    assert torch.allclose(dw, want, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ sensitivity
# Disp_vgg_BN's layer families (the census of tests/test_gpu_nyu_shapes.py): K = input channels x taps per output
FAMILIES = [("conv1_1_K27", [(3, False, False)], 64, False),
            ("enc64_K576", [(64, False, True)], 64, False),
            ("enc128_K1152", [(128, False, True)], 128, False),
            ("enc256_K2304", [(256, False, True)], 64, False),
            ("enc512_K4608", [(512, False, True)], 64, False),
            ("iconv4_K6912", [(256, False, False), (512, False, False)], 32, False),
            ("iconv3_K3456", [(128, False, False), (256, False, False)], 32, False),
            ("iconv2_K1737", [(64, False, False), (128, False, False), (1, True, False)], 64, False),
            ("iconv1_K873", [(32, False, False), (64, False, False), (1, True, False)], 32, False),
            ("iconv0_K153", [(16, False, False), (1, True, False)], 16, False),
            ("head_K144", [(16, False, False)], 1, False),
            ("upconv4_K2048", [(512, False, False)], 64, True),
            ("upconv0_K128", [(32, False, False)], 16, True)]
# ... and those of Disp_res_50, monodepth2 (ResnetEncoder(50) + DepthDecoder) and PoseExpNet (the census of
# tests/test_gpu_zoo_shapes.py); the input gradient's K is Cout x taps of the same family
ZOO_FAMILIES = [("res_stem7x7s2_K147", [(3, False, False, True)], 64, False, (7, 2, 3, 0, False)),
                ("res1x1_K64", [(64, False, True)], 64, False, (1, 1, 0, 0, False)),
                ("res1x1_K256", [(256, False, False)], 64, False, (1, 1, 0, 0, False)),
                ("res1x1s2_K1024", [(1024, False, False)], 64, False, (1, 2, 0, 0, False)),
                ("res1x1_K2048", [(2048, False, False)], 32, False, (1, 1, 0, 0, False)),
                ("res3x3s2_K4608", [(512, False, True)], 32, False, (3, 2, 1, 0, False)),
                ("res_iconv5_K11520", [(256, False, False), (1024, False, False)], 32, False),
                ("res_upconv5_from2048", [(2048, False, False)], 32, True, (3, 2, 1, 1, False)),
                ("res_upconv1_K288", [(32, False, False)], 16, True, (3, 2, 1, 1, False)),
                ("pose_conv1_7x7s2_K441", [(3, False, False, True), (3, False, False, True), (3, False, False, True)], 16, False,
                 (7, 2, 3, 0, False)),
                ("pose_conv2_5x5s2_K400_dgradK800", [(16, False, False)], 32, False, (5, 2, 2, 0, False)),
                ("md2_reflect_K18432", [(2048, False, False)], 32, False, (3, 1, 1, 0, True)),
                ("md2_reflect_up_skip_K11520", [(256, True, False), (1024, False, False)], 32, False, (3, 1, 1, 0, True)),
                ("md2_reflect_up_skip_K864", [(32, True, False), (64, False, False)], 32, False, (3, 1, 1, 0, True)),
                ("md2_reflect_up_K144", [(16, True, False)], 16, False, (3, 1, 1, 0, True)),
                ("md2_dispconv_reflect_K144", [(16, False, False)], 1, False, (3, 1, 1, 0, True))]
ALL_FAMILIES = FAMILIES + ZOO_FAMILIES
# largest pixel count a weight gradient of these families reduces over in the census (b16 x 480 x 640: the stems' output at full
# resolution for Disp_vgg_BN; b32 x 256 x 352 before the zoo shapes)
P_MAX = 16 * 480 * 640
MUTATIONS = ["tap_shifted", "input_channel_dropped", "piece_permuted", "last_row_zeroed"]
# replicate instead of reflect: the padded border repeats the edge row / column (only where the layer reflects)
REFLECT_MUTATION = "border_replicated"


def _case(fam):
    spec, cout, tr, gm = fam[1], fam[2], fam[3], _gm(fam)
    g = torch.Generator().manual_seed(11)
    N, H, W = 3, 8, 12
    pieces = _pieces(g, spec, N, H, W)
    cin = sum(sp[0] for sp in spec)
    w, b = _weights(g, tr, cin, cout, torch.float32, R=gm[0])
    geo = _geo_of(gm, tr, N, H, W, cin, cout)
    return pieces, cin, w, b, geo, g


def _skip(fam, pieces, mutation):
    if mutation == "piece_permuted" and all(p.C == 1 for p in pieces):
        pytest.skip("no multi-channel piece")
    if mutation == REFLECT_MUTATION and not _gm(fam)[4]:
        pytest.skip("no reflection padding")


def _shift_tap(w, tr):
    """Weights of the centre-ish tap only, and the rest."""
    r = s = min(1, w.shape[2] - 1)
    only = torch.zeros_like(w)
    only[:, :, r, s] = w[:, :, r, s]
    return only, w - only


def _shift_cols(x):
    """x [N, C, H, W] read one column to the right (zero beyond the border)."""
    return F.pad(x[..., 1:], (0, 1))


def _permute_piece(x, pieces):
    """Channels of the first multi-channel piece rolled by one (NCHW)."""
    c0 = 0
    for p in pieces:
        if p.C > 1:
            x = x.clone()
            x[:, c0:c0 + p.C] = torch.roll(x[:, c0:c0 + p.C], 1, dims=1)
            return x
        c0 += p.C
    raise AssertionError("no multi-channel piece")


def _fwd_fp32(pieces, w, b, tr, mutation=None, gm=None):
    leaves = [_logical(p, torch.float32) for p in pieces]
    x = _input(leaves, pieces)
    if mutation == "input_channel_dropped":
        x = x.clone()
        x[:, x.shape[1] // 2] = 0
    if mutation == "piece_permuted":
        x = _permute_piece(x, pieces)
    if mutation == "tap_shifted":
        only, rest = _shift_tap(w, tr)
        y = _torch_conv(x, rest, b, tr, gm) + _torch_conv(_shift_cols(x), only, None, tr, gm)
    else:
        y = _torch_conv(x, w, b, tr, gm, "replicate" if mutation == REFLECT_MUTATION else "reflect")
    if mutation == "last_row_zeroed":
        y = y.clone()
        y[:, :, -1] = 0
    return y.permute(0, 2, 3, 1)


def _dgrad_fp32(dy, w, tr, pieces, mutation=None, geo=None):
    """fp32 input gradient [N, IH, IW, Cin] of the concatenated input; dy [N, Cout, OH, OW]."""
    def grad(d, ww):
        if geo is None:
            return F.conv2d(d, ww, stride=2, padding=1) if tr else F.conv_transpose2d(d, ww, padding=1)
        st, pad = geo["stride"], geo["pad"]
        if tr:
            return F.conv2d(d, ww, stride=st, padding=pad)
        if not geo["reflect"]:
            op = geo["IH"] - ((d.shape[2] - 1) * st - 2 * pad + geo["R"])
            return F.conv_transpose2d(d, ww, stride=st, padding=pad, output_padding=op)
        # the gradient of the padded operand, its border folded back in fp32 through the padding's own adjoint
        gp = F.conv_transpose2d(d, ww, stride=st)
        x0 = torch.zeros((d.shape[0], ww.shape[1], geo["IH"], geo["IW"]), requires_grad=True)
        xp = F.pad(x0, (pad,) * 4, mode="replicate" if mutation == REFLECT_MUTATION else "reflect")
        return torch.autograd.grad(xp, x0, gp)[0]
    if mutation == "input_channel_dropped":        # one channel of the reduction (an output channel of the forward) lost
        dy = dy.clone()
        dy[:, dy.shape[1] // 2] = 0
    if mutation == "tap_shifted":
        only, rest = _shift_tap(w, tr)
        dx = grad(dy, rest) + grad(_shift_cols(dy), only)
    else:
        dx = grad(dy, w)
    if mutation == "piece_permuted":
        dx = _permute_piece(dx, pieces)
    if mutation == "last_row_zeroed":
        # the last row the gradient reaches (a 1 x 1 stride-2 convolution never reads the last of an even number of rows)
        last = -1
        if geo is not None and not tr and not geo["reflect"]:
            last = min(geo["IH"] - 1, (geo["OH"] - 1) * geo["stride"] - geo["pad"] + geo["R"] - 1)
        dx = dx.clone()
        dx[:, :, last] = 0
    return dx.permute(0, 2, 3, 1)


def _reflect_mutation(f):
    """The reflection's mutation where it changes the operand: a nearest x2 up-shifted piece has equal edge and next rows, so
    replicate and reflect agree on it -- an operand made only of such pieces cannot tell them apart."""
    return [REFLECT_MUTATION] if _gm(f)[4] and not all(sp[1] for sp in f[1]) else []


FAMILY_MUTATIONS = [(f, m) for f in ALL_FAMILIES for m in [None] + MUTATIONS + _reflect_mutation(f)]


def _fm_id(fm):
    return "%s-%s" % (fm[0][0], fm[1])


@pytest.mark.parametrize("fm", FAMILY_MUTATIONS, ids=[_fm_id(fm) for fm in FAMILY_MUTATIONS])
def test_forward_bound_accepts_fp32_and_rejects_mutations(fm):
    fam, mutation = fm
    pieces, cin, w, b, geo, _g = _case(fam)
    _skip(fam, pieces, mutation)
    X, Xm = CA.Audit._operands(pieces)
    ref = CA.fwd_ref(geo, X, w.double(), b.double())
    A = CA.fwd_ref(geo, Xm, w.double().abs(), b.double().abs())
    got = _fwd_fp32(pieces, w, b, fam[3], mutation, _gm(fam))
    if mutation is None:           # honest fp32: accepted by the tightest family's bound
        ok, worst, rel, over = CA.compare(got, ref, A, CA.C_DIRECT)
        assert ok, (worst, rel, over)
    else:                          # rejected even by the loosest family's bound
        ok, worst, rel, over = CA.compare(got, ref, A, max(CA.C_DIRECT, CA.C_WINO))
        assert not ok and over > 0, (mutation, worst, rel)


@pytest.mark.parametrize("fm", FAMILY_MUTATIONS, ids=[_fm_id(fm) for fm in FAMILY_MUTATIONS])
def test_input_gradient_bound_accepts_fp32_and_rejects_mutations(fm):
    fam, mutation = fm
    pieces, cin, w, b, geo, g = _case(fam)
    _skip(fam, pieces, mutation)
    dy = torch.randn((geo["N"], geo["Cout"], geo["OH"], geo["OW"]), generator=g)
    dY = dy.permute(0, 2, 3, 1).double()
    ref = CA.dgrad_ref(geo, dY, w.double())
    A = CA.dgrad_ref(geo, dY.abs(), w.double().abs())
    got = _dgrad_fp32(dy, w, fam[3], pieces, mutation, geo)
    if mutation is None:
        ok, worst, rel, over = CA.compare(got, ref, A, CA.C_DIRECT)
        assert ok, (worst, rel, over)
    else:
        ok, worst, rel, over = CA.compare(got, ref, A, max(CA.C_DIRECT, CA.C_WINO))
        assert not ok and over > 0, (mutation, worst, rel)


WGRAD_MUTATIONS = ["tap_shifted", "pixel_share_dropped", "last_row_zeroed"]


WGRAD_FAMILY_MUTATIONS = [(f, m) for f in [f for f in FAMILIES if sum(sp[0] for sp in f[1]) <= 256] + ZOO_FAMILIES
                          for m in [None] + WGRAD_MUTATIONS + _reflect_mutation(f)]


@pytest.mark.parametrize("fm", WGRAD_FAMILY_MUTATIONS, ids=[_fm_id(fm) for fm in WGRAD_FAMILY_MUTATIONS])
def test_weight_gradient_bound_accepts_fp32_and_rejects_mutations(fm):
    """The weight gradient's bound grows with the pixels reduced over (conv_audit.bound); it is evaluated at the census's largest
    count, P_MAX, while the data here is small -- so the rejections shown hold with the loosest c any audited call gets."""
    fam, mutation = fm
    pieces, cin, w, b, geo, g = _case(fam)
    N = geo["N"]
    dy = torch.randn((N, geo["OH"], geo["OW"], geo["Cout"]), generator=g)
    chans = sorted({0, cin // 3, cin // 2, cin - 1})
    X32, _ = CA.Audit._operands(pieces, channels=chans)
    X, Xm = CA.Audit._operands(pieces, channels=chans)
    X32 = X32.float()
    ref = CA.wgrad_ref(geo, X, dy.double())
    A = CA.wgrad_ref(geo, Xm, dy.double().abs())
    if mutation == "tap_shifted":
        t = min(1, geo["R"] - 1)
        got = CA.wgrad_ref(geo, X32, dy)
        shifted = CA.wgrad_ref(geo, F.pad(X32[:, :, 1:], (0, 0, 0, 1)), dy)
        got[:, :, t, t] = shifted[:, :, t, t]
    elif mutation == REFLECT_MUTATION:
        p = geo["pad"]
        Xr = F.pad(X32.permute(0, 3, 1, 2), (p,) * 4, mode="replicate").permute(0, 2, 3, 1)
        got = CA.wgrad_ref(dict(geo, reflect=False, pad=0), Xr, dy)
    elif mutation == "pixel_share_dropped":
        splits = 8                                       # one of 8 pixel shares (the largest split count) lost
        keep = torch.ones(N * geo["OH"] * geo["OW"] if not fam[3] else N * geo["IH"] * geo["IW"])
        keep[: keep.numel() // splits] = 0
        if fam[3]:
            got = CA.wgrad_ref(geo, X32 * keep.reshape(N, geo["IH"], geo["IW"], 1), dy)
        else:
            got = CA.wgrad_ref(geo, X32, dy * keep.reshape(N, geo["OH"], geo["OW"], 1))
    else:
        got = CA.wgrad_ref(geo, X32, dy)
        if mutation == "last_row_zeroed":
            got[..., -1, :] = 0
    if mutation is None:
        ok, worst, rel, over = CA.compare(got, ref, A, CA.bound("dn::igemm_wgrad", "wgrad", N * geo["OH"] * geo["OW"]))
        assert ok, (worst, rel, over)
    else:
        ok, worst, rel, over = CA.compare(got, ref, A, CA.bound("dn::wino_wgrad", "wgrad", P_MAX))
        assert not ok and over > 0, (mutation, worst, rel)


def test_bound_is_tight_enough_to_see_one_dropped_term():
    """One term of K = 576 is ~A / 576 = 2.9e4 u A: every fwd / dgrad c sits far below it."""
    for kernel in ("dn::igemm_conv_kernel", "dn::wino_conv8_kernel", "dn::lds3_conv_kernel"):
        for pas in ("fwd", "dgrad"):
            assert CA.bound(kernel, pas) <= 2 ** 24 / 6912 / 8, (kernel, pas)
    # ... and at the largest K of the zoo census: DepthDecoder's upconv(4, 0), 2048 channels x 9 taps (one term ~ 910 u A)
    for kernel in ("dn::igemm_conv_kernel", "dn::wino_conv8_kernel", "dn::lds3k_conv_kernel", "dn::stemk_conv_kernel",
                   "dn::ord_head_fwd_kernel"):
        for pas in ("fwd", "dgrad"):
            assert CA.bound(kernel, pas) <= 2 ** 24 / 18432 / 8, (kernel, pas)


def test_host_threads_respect_the_cap(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert CA.host_threads() == 16
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    assert CA.host_threads() == 4
