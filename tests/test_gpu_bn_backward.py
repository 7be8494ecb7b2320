"""The BatchNorm backward's apply pass (csrc/dn_bn.hip) through its entry points, on a few thousand elements (pytest -m gpu).

Every form of the pass -- plain or hoisted loop, gradient given as dz / under a pending ReLU / through the 2x2 max-pool -- evaluates
dy = gamma * invstd * (dz - sum(dz) / n - xhat * sum(dz * xhat) / n) with one device function, so the same element must come out with
the same BITS whichever kernel handles it: the comparisons below use torch.equal, no tolerance.  One comparison against fp64 keeps
"equal" from meaning "equally wrong"."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from supervised_dispnet_amd import _lib, engine  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _last_kernel():
    return _lib.load().dn_last_kernel().decode()


def _params(C, gen=None):
    """Per-channel BatchNorm state of order 1 (invstd <= 10).  gen None: the same values in every channel."""
    if gen is None:
        mean, invstd, gamma, beta = (torch.full((C,), v, device=DEV) for v in (0.1, 1.7, 0.9, 0.05))
    else:
        mean = torch.randn(C, device=DEV, generator=gen) * 0.3
        invstd = torch.rand(C, device=DEV, generator=gen) * 2.0 + 0.5
        gamma = torch.rand(C, device=DEV, generator=gen) * 0.8 + 0.6
        beta = torch.randn(C, device=DEV, generator=gen) * 0.2
    scale = gamma * invstd
    return types.SimpleNamespace(mean=mean, invstd=invstd, gamma=gamma, scale=scale, shift=beta - mean * scale)


def _apply(g, y, p, partial, relu):
    """dn_bn_bwd_apply_relu (g = da) or dn_bn_bwd_apply (g = dz) on a copy of g: (dy, dgamma, dbeta, the kernel that ran)."""
    rows, C = g.shape
    dy = g.clone()
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    sums = (partial.data_ptr(), partial.shape[0], 2, 0, rows, C, dg.data_ptr(), db.data_ptr(), _stream())
    if relu:
        _lib.call("dn_bn_bwd_apply_relu", dy.data_ptr(), y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), p.mean.data_ptr(),
                  p.invstd.data_ptr(), p.gamma.data_ptr(), *sums)
    else:
        _lib.call("dn_bn_bwd_apply", dy.data_ptr(), y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr(), p.gamma.data_ptr(), *sums)
    return dy, dg, db, _last_kernel()


def _assert_fp64(dy, z, y, p, dg, db):
    """|dy - gamma invstd (z - db / n - xhat dg / n)| <= 8 u |gamma invstd| (|z| + |db / n| + |xhat dg / n|) per element, the reference
    in fp64 from the fp32 operands and the (dgamma, dbeta) the call handed back: the kernel makes six correctly rounded fp32 operations
    per element (xhat: a difference and a product; two fused multiply-adds; xhat * dgamma; gamma * invstd; the final product is the
    seventh, and 1 / n is rounded once), each at most u relative to a quantity the bracket bounds -- 8 leaves slack."""
    n = float(dy.shape[0])
    z, y, dg, db = z.double(), y.double(), dg.double(), db.double()
    k = p.gamma.double() * p.invstd.double()
    xhat = (y - p.mean.double()) * p.invstd.double()
    ref = k * (z - db / n - xhat * dg / n)
    bound = 8 * U * k.abs() * (z.abs() + (db / n).abs() + (xhat * dg / n).abs())
    err = (dy.double() - ref).abs()
    assert bool((err <= bound).all()), "worst error / bound: %.3f" % float((err / bound).max())


# (C, the loop the launcher picks): one block of hoisted; the grid rounded to a multiple of 3 blocks (the lcm path); rounding would
# take 65 blocks > 64, so the plain loop
LOOPS = [(16, "hoisted"), (12, "hoisted"), (260, "plain")]


@pytest.mark.parametrize("rows", [37, 1030])      # 1030: the hoisted loop's four-in-flight tail (i < total false for some u)
def test_plain_loop_is_bitwise_the_hoisted_loop(rows):
    gen = torch.Generator(device=DEV).manual_seed(rows)
    col_g = torch.randn(rows, 1, device=DEV, generator=gen)
    col_y = torch.randn(rows, 1, device=DEV, generator=gen) * 0.6 + 0.1
    first = {}
    for C, loop in LOOPS:
        p = _params(C)
        g, y = col_g.expand(rows, C).contiguous(), col_y.expand(rows, C).contiguous()
        pre = y.double() * p.scale.double() + p.shift.double()
        assert float(pre.abs().min()) > 1e-5         # no element at the edge of the ReLU: the fp64 mask below is the kernel's
        for relu in (False, True):
            z = torch.where(pre > 0, g, torch.zeros_like(g)) if relu else g
            xhat = (y.double() - p.mean.double()) * p.invstd.double()
            # ONE partial row: the column sum is that row, exact in any order
            partial = torch.stack([z.double().sum(0), (z.double() * xhat).sum(0)], dim=1).float().reshape(1, C, 2).contiguous()
            dy, dg, db, kernel = _apply(g, y, p, partial, relu)
            torch.cuda.synchronize()
            assert kernel == "dn::bn_bwd_apply%s_kernel<%s>" % ("_hoisted" if loop == "hoisted" else "", "true" if relu else "false")
            assert torch.equal(dg, partial[0, :, 1]) and torch.equal(db, partial[0, :, 0])
            assert torch.equal(dy, dy[:, :1].expand_as(dy))        # every channel carries the same column
            if C == 16:
                _assert_fp64(dy, z, y, p, dg, db)
            got = (dy[:, 0].clone(), dg[0].clone(), db[0].clone())
            want = first.setdefault(relu, got)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), "C=%d relu=%s" % (C, relu)


@pytest.mark.parametrize("rows,C", [(37, 16), (37, 260), (37, 12), (1030, 12)])
def test_relu_form_is_bitwise_the_dz_form_on_a_premasked_gradient(rows, C):
    gen = torch.Generator(device=DEV).manual_seed(100 * rows + C)
    p = _params(C, gen)                                               # channels differ: a wrong channel group shows
    da = torch.randn(rows, C, device=DEV, generator=gen)
    y = torch.randn(rows, C, device=DEV, generator=gen) * 0.6 + p.mean
    nblk = _lib.load().dn_reduce_blocks(rows, C)
    partial = torch.empty(nblk, C, 2, device=DEV)
    dz = da.clone()
    _lib.call("dn_bn_relu_bwd_reduce", dz.data_ptr(), y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), p.mean.data_ptr(),
              p.invstd.data_ptr(), rows, C, partial.data_ptr(), _stream())
    a = _apply(da, y, p, partial, True)
    b = _apply(dz, y, p, partial, False)
    torch.cuda.synchronize()
    assert 0 < int((dz == 0).sum()) < dz.numel()                      # the mask did something
    assert a[3] == b[3].replace("<false>", "<true>")
    for ta, tb in zip(a[:3], b[:3]):
        assert torch.equal(ta, tb)
    _assert_fp64(a[0], dz, y, p, a[1], a[2])


def test_pool_form_is_bitwise_the_dz_form():
    N, H, W, C = 2, 6, 4, 12
    gen = torch.Generator(device=DEV).manual_seed(7)
    p = _params(C, gen)
    y = torch.randn(N, H, W, C, device=DEV, generator=gen) * 0.6 + p.mean
    pooled = torch.empty(N, H // 2, W // 2, C, device=DEV)
    idx = torch.empty(N, H // 2, W // 2, C, dtype=torch.uint8, device=DEV)
    _lib.call("dn_bn_relu_pool_fwd", y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), N, H, W, C, pooled.data_ptr(), idx.data_ptr(), _stream())
    dpooled = torch.randn(pooled.shape, device=DEV, generator=gen)
    prow = _lib.load().dn_reduce_blocks(N * (H // 2) * (W // 2), C)
    stats = (y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr())
    # A: the materialised dz and its sums, then the dz form
    dz = torch.full((N, H, W, C), float("nan"), device=DEV)
    partial_a = torch.empty(prow, C, 2, device=DEV)
    _lib.call("dn_bn_relu_pool_bwd", dpooled.data_ptr(), idx.data_ptr(), *stats, N, H, W, C, dz.data_ptr(), partial_a.data_ptr(), _stream())
    dy_a, dg_a, db_a, _ = _apply(dz.reshape(-1, C), y.reshape(-1, C), p, partial_a, False)
    # B: the sums alone, then the pool form expands (dpooled, idx) itself
    partial_b = torch.empty(prow, C, 2, device=DEV)
    _lib.call("dn_bn_relu_pool_bwd_sums", dpooled.data_ptr(), idx.data_ptr(), *stats, N, H, W, C, partial_b.data_ptr(), _stream())
    dy_b = torch.full((N, H, W, C), float("nan"), device=DEV)
    dg_b, db_b = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    _lib.call("dn_bn_bwd_apply_pool", dpooled.data_ptr(), idx.data_ptr(), *stats, p.gamma.data_ptr(), partial_b.data_ptr(), prow, 2, 0,
              N, H, W, C, dy_b.data_ptr(), dg_b.data_ptr(), db_b.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dz).all()) and 0 < int((dz != 0).sum()) <= dpooled.numel()
    assert torch.equal(partial_a, partial_b)
    assert torch.equal(dy_a, dy_b.reshape(-1, C))
    assert torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b)


def test_a_second_writer_of_the_gradient_drops_the_sums():
    """Host logic only: Act.grad_dest() hands the first writer a fresh tensor and keeps sums taken alongside; the second call is an
    accumulation, after which those sums no longer describe the gradient."""
    a = engine.Act(torch.zeros(1, 2, 2, 4, device=DEV), 1, 2, 2, 4)
    a.bn_sums = engine.BnSums(torch.zeros(1, 4, 2, device=DEV), 1)
    g, accumulate = a.grad_dest()
    assert g is a.grad and not accumulate and a.bn_sums is not None
    g2, accumulate = a.grad_dest()
    assert g2 is g and accumulate and a.bn_sums is None
