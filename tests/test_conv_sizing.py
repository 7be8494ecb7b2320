"""Host-only sizing entry points against recorded values: dn_conv_wgrad_workspace_bytes, dn_conv_packed_weight_elems and
dn_conv_splitk_workspace_bytes for every convolution call of the networks below, at 4 and 32 images.  No GPU: the library loads and
plans without one (tests/test_abi_and_plan.py).

Why: a caller brings the weight-gradient workspace dn_conv_wgrad_workspace_bytes asks for, and dn_conv2d_wgrad silently falls to a
slower kernel family when that is less than the family needs -- the sizing side and the launch side read the same family table in
dn_conv.hip, and this test pins what the table (and the split plan and the tap windows behind it) yields.  The size is a maximum over
the eligible families, so the list reaches every one of them: the one-channel heads, the Winograd layers of the encoders / decoders,
lds3 (iconv0, the first encoder layer), lds3k (iconv1), stemk (the 7x7 / stride-2 stems on planar images), thin (a 3 -> 16 first
layer read as NHWC), the 64 + 128 + 1 and 64 + 256 + 1 iconv inputs (leading pieces + trailing channel) and the 49-tap stems (tap
windows); test_each_switchable_family_sizes_some_descriptor shows it for the families that have a switch.

tests/golden/conv_sizing.json was recorded by running this module as a script against the library built from the commit BEFORE the
family table was introduced:

    DISPNET_HIP_LIB=<that build's libdispnet_hip.so> python tests/test_conv_sizing.py --record

and is only to be re-recorded, the same way, by a change that means to alter a size.  Equality is exact.

Routes.  Which forward family (row of kConvFamilies in dn_conv.hip) takes a forward / input-gradient / conv-transpose call decides the
launch, the packed weight layout and what the host queries promise the engine (a reciprocal written, statistics finished).
tests/golden/conv_routes.json pins dn_debug_conv_route for the same descriptor list: {switch: {key: [forward route, input-gradient
route]}} with the switch "default" (none set) or one of ROUTE_SWITCHES.  It was recorded against the library built from the commit
BEFORE that table was introduced, which decided by a chain of if statements in run_conv; that build carried one addition,
dn_debug_conv_route written as a literal copy of the chain with `return "name"` in place of each launch (and reported the ABI version
of its day, which the recording run told the binding to expect):

    DISPNET_HIP_LIB=<that build's libdispnet_hip.so> python tests/test_conv_sizing.py --record-routes

Re-record only in a change that means to move a layer from one family to another.
"""
import ctypes as C
import json
import pathlib
import re
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "conv_sizing.json"
ROUTE_GOLDEN = ROOT / "tests" / "golden" / "conv_routes.json"
ROUTES = ("head_fwd", "head_dgrad", "winograd", "stem3", "stemk", "stem", "lds3", "lds3k", "thin", "tiled")    # the rows of kConvFamilies
ROUTE_SWITCHES = ("DN_NO_WINOGRAD", "DN_NO_DIRECT", "DN_NO_LDS3", "DN_NO_THIN_CONV")
BATCHES = (4, 32)


# ------------------------------------------------------------------------------------------------------------ the calls
# One conv call: (name, transposed, k, stride, pad, pieces, cout, (IH, IW), (OH, OW)); a piece: (C, flags) with flags out of
# "u" nearest x2 up-shift, "a" pending BatchNorm scale / shift, "p" planar (NCHW) image.
def _conv(name, k, s, p, pieces, cout, hw):
    oh, ow = (hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1
    return (name, False, k, s, p, [pc if isinstance(pc, tuple) else (pc, "") for pc in pieces], cout, hw, (oh, ow))


def _convT(name, k, p, cin, cout, hw, out_hw):
    return (name, True, k, 2, p, [(cin, "")], cout, hw, out_hw)


def vgg_bn(H, W):
    calls, c, hw = [], 3, (H, W)
    for stage in ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512)):
        for i, v in enumerate(stage):
            flags = "p" if c == 3 else ("a" if i else "")              # a stage's first layer reads the pooled (plain) activation
            calls.append(_conv("enc%d_%dx%d.%d" % (v, hw[0], hw[1], i), 3, 1, 1, [(c, flags)], v, hw))
            c = v
        hw = (hw[0] // 2, hw[1] // 2)
    skips = {16: 512, 8: 256, 4: 128, 2: 64}
    c = 512
    for lvl, cout in ((16, 256), (8, 128), (4, 64), (2, 32), (1, 16)):
        up = (H // lvl, W // lvl)
        calls.append(_convT("upconv@%dx%d" % up, 4, 1, c, cout, (up[0] // 2, up[1] // 2), up))
        pieces = [cout] + ([skips[lvl]] if lvl in skips else []) + ([(1, "u")] if lvl <= 4 else [])
        calls.append(_conv("iconv@%dx%d" % up, 3, 1, 1, pieces, cout, up))
        if lvl <= 8:
            calls.append(_conv("disp@%dx%d" % up, 3, 1, 1, [cout], 1, up))
        c = cout
    return calls


def res50(H, W):
    calls = [_conv("conv1", 7, 2, 3, [(3, "p")], 64, (H, W))]
    hw, inpl = (H // 4, W // 4), 64
    for li, (planes, n, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)), start=1):
        for b in range(n):
            s = stride if b == 0 else 1
            out = (hw[0] // s, hw[1] // s)
            tag = "layer%d.%d." % (li, b)
            calls.append(_conv(tag + "conv1", 1, 1, 0, [inpl], planes, hw))
            calls.append(_conv(tag + "conv2", 3, s, 1, [(planes, "a")], planes, hw))
            calls.append(_conv(tag + "conv3", 1, 1, 0, [(planes, "a")], planes * 4, out))
            if b == 0:
                calls.append(_conv(tag + "ds", 1, s, 0, [inpl], planes * 4, hw))
            inpl, hw = planes * 4, out
    c = 2048
    for lvl, cout, skip, disp in ((16, 256, 1024, False), (8, 128, 512, False), (4, 64, 256, True), (2, 32, 64, True), (1, 16, 0, True)):
        up = (H // lvl, W // lvl)
        calls.append(_convT("upconv@%dx%d" % up, 3, 1, c, cout, (up[0] // 2, up[1] // 2), up))
        calls.append(_conv("iconv@%dx%d" % up, 3, 1, 1, [cout] + ([skip] if skip else []) + ([(1, "u")] if disp else []), cout, up))
        if lvl <= 8:
            calls.append(_conv("disp@%dx%d" % up, 3, 1, 1, [cout], 1, up))
        c = cout
    return calls


def dispnets(H, W):
    calls, c, hw, sizes = [], 3, (H, W), [(H, W)]
    cp = (32, 64, 128, 256, 512, 512, 512)
    for i, (v, k) in enumerate(zip(cp, (7, 5, 3, 3, 3, 3, 3)), start=1):
        calls.append(_conv("conv%d.0" % i, k, 2, (k - 1) // 2, [(c, "p" if c == 3 else "")], v, hw))
        hw = calls[-1][8]
        calls.append(_conv("conv%d.2" % i, k, 1, (k - 1) // 2, [v], v, hw))
        sizes.append(hw)
        c = v
    for i, cout in zip(range(7, 0, -1), (512, 512, 256, 128, 64, 32, 16)):
        out = sizes[i - 1]
        calls.append(_convT("upconv%d" % i, 3, 1, c, cout, sizes[i], out))                     # (output_padding 1, cropped to the skip)
        calls.append(_conv("iconv%d" % i, 3, 1, 1, [cout] + ([cp[i - 2]] if i >= 2 else []) + ([1] if i <= 3 else []), cout, out))
        if i <= 4:
            calls.append(_conv("predict_disp%d" % i, 3, 1, 1, [cout], 1, out))
        c = cout
    return calls


def posenet(H, W):
    calls, hw, sizes, c = [], (H, W), [(H, W)], None
    for i, (v, k) in enumerate(zip((16, 32, 64, 128, 256, 256, 256), (7, 5, 3, 3, 3, 3, 3)), start=1):
        calls.append(_conv("conv%d" % i, k, 2, (k - 1) // 2, [(3, "p")] * 3 if c is None else [c], v, hw))
        hw = calls[-1][8]
        sizes.append(hw)
        c = v
    calls.append(_conv("pose_pred", 1, 1, 0, [256], 12, hw))
    c = 256
    for i, cout in zip((5, 4, 3, 2, 1), (256, 128, 64, 32, 16)):
        calls.append(_convT("upconv%d" % i, 4, 1, c, cout, sizes[i], sizes[i - 1]))
        if i <= 4:
            calls.append(_conv("predict_mask%d" % i, 3, 1, 1, [cout], 2, sizes[i - 1]))
        c = cout
    return calls


def extras(H, W):
    """Shapes outside the networks above that the dispatch treats on their own."""
    return [_conv("first3_nhwc", 3, 1, 1, [3], 64, (H, W)),                                       # a 3-channel first layer read as NHWC
            _conv("first3_16_nhwc", 3, 1, 1, [3], 16, (H, W)),                                    # ... 16 wide: the thin kernel's alone
            _conv("iconv_64_128_1", 3, 1, 1, [64, 128, (1, "u")], 64, (H // 4, W // 4)),
            _conv("iconv_64_256_1", 3, 1, 1, [64, 256, (1, "u")], 64, (H // 4, W // 4)),
            _conv("head_16", 3, 1, 1, [16], 1, (H, W)),
            _conv("head_256", 3, 1, 1, [256], 1, (H // 8, W // 8)),
            _conv("stem7_nhwc", 7, 2, 3, [3], 64, (H, W))]                                        # 49 taps without the planar-image stem kernel


NETS = (("vggbn_128x416", vgg_bn, 128, 416), ("vggbn_256x352", vgg_bn, 256, 352), ("res50_480x640", res50, 480, 640),
        ("dispnets_128x416", dispnets, 128, 416), ("posenet_128x416", posenet, 128, 416), ("extras_128x416", extras, 128, 416),
        ("extras_480x640", extras, 480, 640))


# ------------------------------------------------------------------------------------------------------ descriptors
def _fwd_desc(call, N, compute):
    from supervised_dispnet_amd._lib import ACT_LEAKY, CONV_FWD, CONVT_FWD, ConvDesc
    _, transposed, k, s, p, pieces, cout, (IH, IW), (OH, OW) = call
    d = ConvDesc()
    d.kind = CONVT_FWD if transposed else CONV_FWD
    d.N, d.IH, d.IW, d.OH, d.OW, d.R, d.S, d.stride, d.pad, d.dilation, d.compute = N, IH, IW, OH, OW, k, k, s, p, 1, compute
    d.n_in = len(pieces)
    for i, (c, flags) in enumerate(pieces):
        o = d.in_[i]
        h, w = (IH // 2, IW // 2) if "u" in flags else (IH, IW)
        o.data = (i + 1) << 32                   # fake, 16-byte aligned: host planning only looks at presence / alignment
        o.C, o.up_shift = c, 1 if "u" in flags else 0
        if "p" in flags:
            o.stride_n, o.stride_c, o.stride_h, o.stride_w = c * h * w, h * w, w, 1
        else:
            o.stride_n, o.stride_h, o.stride_w, o.stride_c = h * w * c, w * c, c, 1
        if "a" in flags:
            o.scale, o.shift = (8 << 32) + 4096 * i, (9 << 32) + 4096 * i
    d.n_out = 1
    r = d.out[0]
    r.data, r.C, r.stride_w, r.stride_h, r.stride_n = 12 << 32, cout, cout, OW * cout, OH * OW * cout
    d.w_packed, d.bias, d.act, d.act_p0 = 13 << 32, 14 << 32, ACT_LEAKY, 0.1
    return d


def _dgrad_desc(call, N, compute):
    from supervised_dispnet_amd._lib import CONV_DGRAD, CONVT_DGRAD, ConvDesc
    _, transposed, k, s, p, pieces, cout, (IH, IW), (OH, OW) = call
    d = ConvDesc()
    d.kind = CONVT_DGRAD if transposed else CONV_DGRAD
    d.N, d.IH, d.IW, d.OH, d.OW, d.R, d.S, d.stride, d.pad, d.dilation, d.compute = N, OH, OW, IH, IW, k, k, s, p, 1, compute
    d.n_in = 1
    o = d.in_[0]
    o.data, o.C = 1 << 32, cout
    o.stride_c, o.stride_w, o.stride_h, o.stride_n = 1, cout, OW * cout, OH * OW * cout
    d.n_out = len(pieces)
    for i, (c, _flags) in enumerate(pieces):
        r = d.out[i]                            # (the gradient of an up-shifted piece is taken at the full extent and folded afterwards)
        r.data, r.C, r.stride_w, r.stride_h, r.stride_n = (i + 2) << 32, c, c, IW * c, IH * IW * c
    d.w_packed = 13 << 32
    return d


def descriptors():
    """[(key, forward descriptor, input-gradient descriptor)] of every call x batch x arithmetic."""
    from supervised_dispnet_amd._lib import COMPUTE_F32, COMPUTE_F32X3
    out = []
    for net, fn, H, W in NETS:
        for call in fn(H, W):
            for N in BATCHES:
                for cname, compute in (("f32x3", COMPUTE_F32X3), ("f32", COMPUTE_F32)):
                    out.append(("%s/%s/b%d/%s" % (net, call[0], N, cname), _fwd_desc(call, N, compute), _dgrad_desc(call, N, compute)))
    assert len({k for k, _, _ in out}) == len(out), "descriptor keys are not unique"
    return out


def measure(lib):
    """key -> [wgrad workspace bytes, packed elems fwd, packed elems dgrad, splitk bytes fwd, splitk bytes dgrad]"""
    got = {}
    for key, f, g in descriptors():
        got[key] = [int(lib.dn_conv_wgrad_workspace_bytes(C.byref(f))), int(lib.dn_conv_packed_weight_elems(C.byref(f))),
                    int(lib.dn_conv_packed_weight_elems(C.byref(g))), int(lib.dn_conv_splitk_workspace_bytes(C.byref(f))),
                    int(lib.dn_conv_splitk_workspace_bytes(C.byref(g)))]
    return got


def routes(lib):
    """key -> [forward route, input-gradient route]"""
    return {key: [lib.dn_debug_conv_route(C.byref(f)).decode(), lib.dn_debug_conv_route(C.byref(g)).decode()] for key, f, g in descriptors()}


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    from supervised_dispnet_amd import _lib
    return _lib.load()


def test_sizing_matches_the_recorded_values(lib):
    want = json.loads(GOLDEN.read_text())
    got = measure(lib)
    assert sorted(got) == sorted(want), "the descriptor list and the recorded list differ"
    for key in sorted(got):
        assert got[key][0] > 0 and got[key][1] > 0 and got[key][2] > 0, "%s: a descriptor the library rejects: %s" % (key, got[key])
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, "%d of %d descriptors size differently (got, recorded): %s" % (len(bad), len(got), sorted(bad.items())[:8])


@pytest.mark.parametrize("switch", ["DN_NO_WINOGRAD_WGRAD", "DN_NO_LDS3", "DN_NO_THIN", "DN_NO_TAP_WINDOWS"])
def test_each_switchable_family_sizes_some_descriptor(lib, monkeypatch, switch):
    """Taking one family out changes the size of at least one descriptor of the list: the list reaches that family's row (DN_NO_LDS3
    covers lds3, lds3k and stemk).  The head and the leading-pieces split have no sizing switch; their descriptors are in the list by
    construction (disp@ / head_*, iconv_64_128_1 / iconv_64_256_1)."""
    base = {k: v[0] for k, v in measure(lib).items()}
    monkeypatch.setenv(switch, "1")
    lib.dn_reload_knobs()
    try:
        off = {k: v[0] for k, v in measure(lib).items()}
    finally:
        monkeypatch.delenv(switch)
        lib.dn_reload_knobs()
    assert any(off[k] != base[k] for k in base), "%s changes no weight-gradient workspace of the list" % switch


@pytest.fixture(params=("default",) + ROUTE_SWITCHES)
def switch(request, lib, monkeypatch):
    if request.param != "default":
        monkeypatch.setenv(request.param, "1")
    lib.dn_reload_knobs()
    yield request.param
    monkeypatch.undo()
    lib.dn_reload_knobs()


def test_the_route_list_is_the_family_table():
    src = (ROOT / "supervised_dispnet_amd" / "csrc" / "dn_conv.hip").read_text()
    table = src[src.index("kConvFamilies[] = {"):]
    table = table[:table.index("\n};")]
    assert tuple(re.findall(r'^    \{"(\w+)",', table, re.M)) == ROUTES


def test_routes_match_the_recorded_values(lib, switch):
    want = json.loads(ROUTE_GOLDEN.read_text())
    assert sorted(want) == sorted(("default",) + ROUTE_SWITCHES)
    got = routes(lib)
    assert sorted(got) == sorted(want[switch]), "the descriptor list and the recorded list differ"
    bad = {k: (got[k], want[switch][k]) for k in got if got[k] != want[switch][k]}
    assert not bad, "%s: %d of %d descriptors route differently (got, recorded): %s" % (switch, len(bad), len(got), sorted(bad.items())[:8])
    if switch == "default":
        # a row the list does not reach would go unpinned (head_dgrad by input gradients only, the stems by forwards only)
        assert {r for v in got.values() for r in v} == set(ROUTES)
    else:
        assert got != want["default"], "%s moves no descriptor of the list" % switch


def test_queries_agree_with_the_route(lib, switch):
    """What the engine acts on (the layout it packs, the reciprocal buffer it allocates, the BatchNorm-backward sums it leaves to the
    input gradient) belongs to the family that will run."""
    for key, f, g in descriptors():
        for d in (f, g):
            route = lib.dn_debug_conv_route(C.byref(d)).decode()
            assert (lib.dn_conv_weight_layout(C.byref(d)) != 0) == (route == "winograd"), key
            assert lib.dn_conv_fwd_fuses_reciprocal(C.byref(d)) != 1 or route == "head_fwd", key
            assert lib.dn_conv_dgrad_fuses_bn_sums(C.byref(d)) != 1 or route == "winograd", key


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    from supervised_dispnet_amd import _lib as _binding
    if "--record-routes" in sys.argv:
        import os
        lib, recorded = _binding.load(), {}
        for sw in ("default",) + ROUTE_SWITCHES:
            os.environ.update({sw: "1"} if sw != "default" else {})
            lib.dn_reload_knobs()
            recorded[sw] = routes(lib)
            os.environ.pop(sw, None)
        ROUTE_GOLDEN.write_text(json.dumps(recorded, indent=0, sort_keys=True, separators=(",", ":")) + "\n")
        sys.exit("recorded %d descriptors x %d switch settings from %s" % (len(recorded["default"]), len(recorded), _binding.LIB_PATH))
    if "--record" not in sys.argv:
        sys.exit("usage: DISPNET_HIP_LIB=<reference build> python tests/test_conv_sizing.py --record | --record-routes")
    values = measure(_binding.load())
    GOLDEN.write_text(json.dumps(values, indent=0, sort_keys=True, separators=(",", ":")) + "\n")
    print("recorded %d descriptors from %s" % (len(values), _binding.LIB_PATH))
