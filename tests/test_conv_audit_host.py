"""Host checks of tests/conv_audit.py, the fp64 audit the GPU tests put around every convolution call (no GPU needed).

  * the audit's fp64 reference of each operand form -- a concat of 2 or 3 pieces, an up-shifted 1-channel piece, a BatchNorm-pending
    affine piece, the 4 x 4 stride-2 transposed convolution, the 3 x 3 convolution -- equals torch fp64 (F.conv2d /
    F.conv_transpose2d / autograd) applied to the independently materialised input, for the forward, the input gradient (folded
    through the up-shift) and the weight gradient;
  * sensitivity: at the K of every layer family Disp_vgg_BN's census shows, the bound accepts an honest fp32 result and rejects it
    after one tap shifted, one input channel dropped, one concat piece's channels permuted, the last output row zeroed -- and, for
    the weight gradient, one 1/splits share of the pixels dropped.  This is the evidence that the GPU audit would fail on a subtly
    wrong kernel.
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


def _piece(g, N, H, W, C, up=False, affine=False):
    """A CPU Act: post-ReLU-like values, or pre-BatchNorm values with a pending (scale, shift) + ReLU."""
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
    x = p.act.t.to(dtype)
    if p.act.scale is not None:
        x = torch.relu(x * p.act.scale.to(dtype) + p.act.shift.to(dtype))
    return x.permute(0, 3, 1, 2)


def _input(leaves, pieces):
    xs = [F.interpolate(x, scale_factor=2, mode="nearest") if p.up else x for x, p in zip(leaves, pieces)]
    return torch.cat(xs, dim=1)


def _geo(transposed, N, IH, IW, Cin, Cout):
    if transposed:
        return {"N": N, "IH": IH, "IW": IW, "OH": 2 * IH, "OW": 2 * IW, "R": 4, "S": 4, "stride": 2, "pad": 1, "dil": 1, "transposed": True,
                "Cin": Cin, "Cout": Cout}
    return {"N": N, "IH": IH, "IW": IW, "OH": IH, "OW": IW, "R": 3, "S": 3, "stride": 1, "pad": 1, "dil": 1, "transposed": False,
            "Cin": Cin, "Cout": Cout}


def _weights(g, transposed, cin, cout, dtype=torch.float64):
    shape = (cin, cout, 4, 4) if transposed else (cout, cin, 3, 3)
    rf = shape[2] * shape[3]
    b = (6.0 / ((cin + cout) * rf)) ** 0.5
    return ((torch.rand(shape, generator=g) * 2 - 1) * b).to(dtype), ((torch.rand(cout, generator=g) * 2 - 1) * 0.05).to(dtype)


def _torch_conv(x, w, b, transposed):
    return F.conv_transpose2d(x, w, b, stride=2, padding=1) if transposed else F.conv2d(x, w, b, padding=1)


# (id, piece list [(channels, up, affine)], Cout, transposed)
FORMS = [("conv3x3_affine", [(24, False, True)], 16, False),
         ("concat2", [(16, False, False), (24, False, True)], 8, False),
         ("concat3_with_up1", [(8, False, False), (16, False, False), (1, True, False)], 8, False),
         ("up1_only", [(1, True, False)], 4, False),
         ("convT4x4s2_affine", [(12, False, True)], 8, True)]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_reference_matches_torch_fp64_on_the_materialised_input(form):
    _tag, spec, cout, tr = form
    g = torch.Generator().manual_seed(3)
    N, H, W = 3, 6, 10
    pieces = [_piece(g, N, H // 2 if up else H, W // 2 if up else W, c, up, aff) for c, up, aff in spec]
    cin = sum(c for c, _, _ in spec)
    w, b = _weights(g, tr, cin, cout)
    geo = _geo(tr, N, H, W, cin, cout)
    leaves = [_logical(p).clone().requires_grad_(True) for p in pieces]
    wl = w.clone().requires_grad_(True)
    y = _torch_conv(_input(leaves, pieces), wl, b, tr)
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
# largest pixel count a weight gradient of these families reduces over in the census (b32 x 256 x 352)
P_MAX = 32 * 256 * 352
MUTATIONS = ["tap_shifted", "input_channel_dropped", "piece_permuted", "last_row_zeroed"]


def _case(fam):
    _tag, spec, cout, tr = fam
    g = torch.Generator().manual_seed(11)
    N, H, W = 3, 8, 12
    pieces = [_piece(g, N, H // 2 if up else H, W // 2 if up else W, c, up, aff) for c, up, aff in spec]
    cin = sum(c for c, _, _ in spec)
    w, b = _weights(g, tr, cin, cout, torch.float32)
    geo = _geo(tr, N, H, W, cin, cout)
    return pieces, cin, w, b, geo, g


def _shift_tap(w, tr):
    """Weights of the centre-ish tap only, and the rest."""
    r = s = 1
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


def _fwd_fp32(pieces, w, b, tr, mutation=None):
    leaves = [_logical(p, torch.float32) for p in pieces]
    x = _input(leaves, pieces)
    if mutation == "input_channel_dropped":
        x = x.clone()
        x[:, x.shape[1] // 2] = 0
    if mutation == "piece_permuted":
        x = _permute_piece(x, pieces)
    if mutation == "tap_shifted":
        only, rest = _shift_tap(w, tr)
        y = _torch_conv(x, rest, b, tr) + _torch_conv(_shift_cols(x), only, None, tr)
    else:
        y = _torch_conv(x, w, b, tr)
    if mutation == "last_row_zeroed":
        y = y.clone()
        y[:, :, -1] = 0
    return y.permute(0, 2, 3, 1)


def _dgrad_fp32(dy, w, tr, pieces, mutation=None):
    """fp32 input gradient [N, IH, IW, Cin] of the concatenated input; dy [N, Cout, OH, OW]."""
    def grad(d, ww):
        return F.conv2d(d, ww, stride=2, padding=1) if tr else F.conv_transpose2d(d, ww, padding=1)
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
        dx = dx.clone()
        dx[:, :, -1] = 0
    return dx.permute(0, 2, 3, 1)


@pytest.mark.parametrize("mutation", [None] + MUTATIONS)
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_forward_bound_accepts_fp32_and_rejects_mutations(fam, mutation):
    pieces, cin, w, b, geo, _g = _case(fam)
    if mutation == "piece_permuted" and all(p.C == 1 for p in pieces):
        pytest.skip("no multi-channel piece")
    X, Xm = CA.Audit._operands(pieces)
    ref = CA.fwd_ref(geo, X, w.double(), b.double())
    A = CA.fwd_ref(geo, Xm, w.double().abs(), b.double().abs())
    got = _fwd_fp32(pieces, w, b, fam[3], mutation)
    if mutation is None:           # honest fp32: accepted by the tightest family's bound
        ok, worst, rel, over = CA.compare(got, ref, A, CA.C_DIRECT)
        assert ok, (worst, rel, over)
    else:                          # rejected even by the loosest family's bound
        ok, worst, rel, over = CA.compare(got, ref, A, max(CA.C_DIRECT, CA.C_WINO))
        assert not ok and over > 0, (mutation, worst, rel)


@pytest.mark.parametrize("mutation", [None] + MUTATIONS)
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_input_gradient_bound_accepts_fp32_and_rejects_mutations(fam, mutation):
    pieces, cin, w, b, geo, g = _case(fam)
    if mutation == "piece_permuted" and all(p.C == 1 for p in pieces):
        pytest.skip("no multi-channel piece")
    dy = torch.randn((geo["N"], geo["Cout"], geo["OH"], geo["OW"]), generator=g)
    dY = dy.permute(0, 2, 3, 1).double()
    ref = CA.dgrad_ref(geo, dY, w.double())
    A = CA.dgrad_ref(geo, dY.abs(), w.double().abs())
    got = _dgrad_fp32(dy, w, fam[3], pieces, mutation)
    if mutation is None:
        ok, worst, rel, over = CA.compare(got, ref, A, CA.C_DIRECT)
        assert ok, (worst, rel, over)
    else:
        ok, worst, rel, over = CA.compare(got, ref, A, max(CA.C_DIRECT, CA.C_WINO))
        assert not ok and over > 0, (mutation, worst, rel)


WGRAD_MUTATIONS = ["tap_shifted", "pixel_share_dropped", "last_row_zeroed"]


@pytest.mark.parametrize("mutation", [None] + WGRAD_MUTATIONS)
@pytest.mark.parametrize("fam", [f for f in FAMILIES if sum(c for c, _, _ in f[1]) <= 256], ids=lambda f: f[0])
def test_weight_gradient_bound_accepts_fp32_and_rejects_mutations(fam, mutation):
    """The weight gradient's bound grows with the pixels reduced over (conv_audit.bound); it is evaluated at the census's largest
    count, P_MAX, while the data here is small -- so the rejections shown hold with the loosest c any audited call gets."""
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
        got = CA.wgrad_ref(geo, X32, dy)
        shifted = CA.wgrad_ref(geo, F.pad(X32[:, :, 1:], (0, 0, 0, 1)), dy)
        got[:, :, 1, 1] = shifted[:, :, 1, 1]
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


def test_host_threads_respect_the_cap(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert CA.host_threads() == 16
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    assert CA.host_threads() == 4
