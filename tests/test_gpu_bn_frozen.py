"""The backward of a FROZEN BatchNorm (csrc/dn_bn.hip, the dn_bn_frozen_* entry points) on a few thousand elements (pytest -m gpu).

With running statistics the backward has no batch-mean terms: dy = (gamma * invstd) * dz, dbeta = sum dz, dgamma = sum dz * xhat.  Every
form -- gradient given as dz, under a pending ReLU, through the fused 2x2 max-pool, the residual tail -- is one pass that writes dy and
leaves per-block partial sums, and evaluates an element with one device function (bn_frozen_bwd_value), so the same element must come out
with the same BITS whichever form handles it: torch.equal, no tolerance.  One comparison against fp64 per form keeps "equal" from
meaning "equally wrong".

Rounded fp32 operations per element in the device function (each correctly rounded, contraction off):
  dy          2   gamma * invstd, then the product with dz                              -> bound (2 + 1) u |k dz|
  dgamma term 3   y - mean, times invstd, times dz                                      -> c = 3 in (rows + c) u sum|term|
  dbeta term  0   dz itself                                                              -> c = 0
  dbias       2   gamma * invstd, times the ROUNDED dbeta (on top of dbeta's own sum)    -> c = 2, term = k dz
The sums meet in fp32 inside a block (at most `rows` additions per channel) and in fp64 across blocks: the standard summation bound
(rows + c) u sum|term| covers them."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from supervised_dispnet_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24
EPS = 1e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _params(C, gen):
    """Per-channel frozen BatchNorm state: running variance in [0.04, 4) so that invstd is of order 1 (0.5 .. 5); scale, shift and invstd
    are what the library itself derives from it (dn_bn_frozen_affine)."""
    rm = torch.randn(C, device=DEV, generator=gen) * 0.3
    rv = (torch.rand(C, device=DEV, generator=gen) * 1.8 + 0.2) ** 2
    gamma = torch.rand(C, device=DEV, generator=gen) * 0.8 + 0.6
    beta = torch.randn(C, device=DEV, generator=gen) * 0.2
    scale, shift, invstd = (torch.empty(C, device=DEV) for _ in range(3))
    _lib.call("dn_bn_frozen_affine", C, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, scale.data_ptr(), shift.data_ptr(),
              invstd.data_ptr(), _stream())
    return types.SimpleNamespace(mean=rm, var=rv, gamma=gamma, beta=beta, scale=scale, shift=shift, invstd=invstd)


def _finalize(partial, p, stride=2, offset=0, bias=True):
    C = partial.shape[1]
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dbias = torch.empty(C, device=DEV) if bias else None
    _lib.call("dn_bn_frozen_finalize", partial.data_ptr(), partial.shape[0], stride, offset, C, p.gamma.data_ptr(), p.invstd.data_ptr(),
              dg.data_ptr(), db.data_ptr(), dbias.data_ptr() if bias else None, _stream())
    return dg, db, dbias


def _dz_form(dz, y, p):
    rows, C = dz.shape
    dy = dz.clone()
    partial = torch.empty(_lib.load().dn_reduce_blocks(rows, C), C, 2, device=DEV)
    _lib.call("dn_bn_frozen_bwd", dy.data_ptr(), y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr(), p.gamma.data_ptr(), rows, C,
              partial.data_ptr(), _stream())
    return dy, partial


def _relu_form(da, y, p):
    rows, C = da.shape
    dy = da.clone()
    partial = torch.empty(_lib.load().dn_reduce_blocks(rows, C), C, 2, device=DEV)
    _lib.call("dn_bn_frozen_bwd_relu", dy.data_ptr(), y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), p.mean.data_ptr(),
              p.invstd.data_ptr(), p.gamma.data_ptr(), rows, C, partial.data_ptr(), _stream())
    return dy, partial


def _assert_fp64(dy, dz, y, p, dg, db, dbias):
    """dy, dgamma, dbeta, dbias against fp64 from the fp32 operands (dz, y, mean, invstd, gamma), bounds as in the module docstring."""
    rows = dz.shape[0]
    dz, y = dz.double(), y.double()
    k = p.gamma.double() * p.invstd.double()
    ref = k * dz
    err = (dy.double() - ref).abs()
    bound = 3 * U * ref.abs()
    assert bool((err <= bound).all()), "dy: worst error / bound %.3f" % float((err / bound.clamp_min(1e-300)).max())
    xhat = (y - p.mean.double()) * p.invstd.double()
    for name, got, term, c in (("dbeta", db, dz, 0), ("dgamma", dg, dz * xhat, 3), ("dbias", dbias, k * dz, 2)):
        if got is None:
            continue
        e = (got.double() - term.sum(0)).abs()
        b = (rows + c) * U * term.abs().sum(0)
        assert bool((e <= b).all()), "%s: worst error / bound %.3f" % (name, float((e / b).max()))


def test_frozen_affine_is_the_eval_affine_and_invstd_matches_fp64():
    """invstd: an addition, a square root, a division -- three correctly rounded operations, bound 4 u; scale / shift bitwise those of
    dn_bn_eval_affine (the same kernel)."""
    C = 260
    p = _params(C, torch.Generator(device=DEV).manual_seed(1))
    sc, sh = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    _lib.call("dn_bn_eval_affine", C, p.gamma.data_ptr(), p.beta.data_ptr(), p.mean.data_ptr(), p.var.data_ptr(), EPS, sc.data_ptr(),
              sh.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(sc, p.scale) and torch.equal(sh, p.shift)
    ref = 1.0 / torch.sqrt(p.var.double() + EPS)
    assert bool(((p.invstd.double() - ref).abs() <= 4 * U * ref).all())
    assert 0.4 < float(p.invstd.min()) and float(p.invstd.max()) < 5.5


@pytest.mark.parametrize("rows", [37, 1030])           # 1030: several rows per thread, a ragged last block
@pytest.mark.parametrize("C", [12, 16, 260])           # a partly filled row of threads; full; more channel groups than one sweep's threads (plain C)
def test_relu_form_is_bitwise_the_dz_form_on_a_premasked_gradient(rows, C):
    gen = torch.Generator(device=DEV).manual_seed(100 * rows + C)
    p = _params(C, gen)
    da = torch.randn(rows, C, device=DEV, generator=gen)
    y = torch.randn(rows, C, device=DEV, generator=gen) * 0.6 + p.mean
    dz = da.clone()                                    # the library's own mask (the train-mode reduce pass writes dz in place)
    scratch = torch.empty(_lib.load().dn_reduce_blocks(rows, C), C, 2, device=DEV)
    _lib.call("dn_bn_relu_bwd_reduce", dz.data_ptr(), y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), p.mean.data_ptr(),
              p.invstd.data_ptr(), rows, C, scratch.data_ptr(), _stream())
    dy_a, part_a = _relu_form(da, y, p)
    dy_b, part_b = _dz_form(dz, y, p)
    fa, fb = _finalize(part_a, p), _finalize(part_b, p)
    torch.cuda.synchronize()
    assert 0 < int((dz == 0).sum()) < dz.numel()       # the mask did something
    assert torch.equal(dy_a, dy_b) and torch.equal(part_a, part_b)
    for ta, tb in zip(fa, fb):
        assert torch.equal(ta, tb)
    dg, db, dbias = fa
    _assert_fp64(dy_a, dz, y, p, dg, db, dbias)
    # the bias gradient is the product the finalize evaluates: (gamma * invstd) * dbeta on the ROUNDED dbeta, two fp32 products
    assert torch.equal(dbias, (p.gamma * p.invstd) * db)
    # without a bias in front nothing is written for it
    dg2, db2, _ = _finalize(part_a, p, bias=False)
    torch.cuda.synchronize()
    assert torch.equal(dg2, dg) and torch.equal(db2, db)


@pytest.mark.parametrize("C", [12, 16])
def test_pool_form_is_bitwise_the_dz_form_on_the_expanded_gradient(C):
    N, H, W = 2, 4, 6
    gen = torch.Generator(device=DEV).manual_seed(7 + C)
    p = _params(C, gen)
    y = torch.randn(N, H, W, C, device=DEV, generator=gen) * 0.6 + p.mean
    pooled = torch.empty(N, H // 2, W // 2, C, device=DEV)
    idx = torch.empty(N, H // 2, W // 2, C, dtype=torch.uint8, device=DEV)
    _lib.call("dn_bn_relu_pool_fwd", y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), N, H, W, C, pooled.data_ptr(), idx.data_ptr(), _stream())
    dpooled = torch.randn(pooled.shape, device=DEV, generator=gen)
    prow = _lib.load().dn_reduce_blocks(N * (H // 2) * (W // 2), C)
    # A: the expanded dz as the train-mode kernel materialises it, then the dz form
    dz = torch.full((N, H, W, C), float("nan"), device=DEV)
    scratch = torch.empty(prow, C, 2, device=DEV)
    _lib.call("dn_bn_relu_pool_bwd", dpooled.data_ptr(), idx.data_ptr(), y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr(), N, H, W, C,
              dz.data_ptr(), scratch.data_ptr(), _stream())
    dy_a, part_a = _dz_form(dz.reshape(-1, C), y.reshape(-1, C), p)
    # B: the pool form expands (dpooled, idx) itself
    dy_b = torch.full((N, H, W, C), float("nan"), device=DEV)
    part_b = torch.empty(prow, C, 2, device=DEV)
    _lib.call("dn_bn_frozen_bwd_pool", dpooled.data_ptr(), idx.data_ptr(), y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr(),
              p.gamma.data_ptr(), N, H, W, C, dy_b.data_ptr(), part_b.data_ptr(), _stream())
    dg, db, dbias = _finalize(part_b, p)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dz).all()) and 0 < int((dz != 0).sum()) <= dpooled.numel()
    assert torch.equal(dy_a, dy_b.reshape(-1, C))
    # (the partial rows partition pooled pixels here and full-resolution pixels there: the sums are compared against fp64, not bitwise)
    _assert_fp64(dy_b.reshape(-1, C), dz.reshape(-1, C), y.reshape(-1, C), p, dg, db, dbias)
    assert torch.equal(dbias, (p.gamma * p.invstd) * db)


@pytest.mark.parametrize("branch", ["downsample", "identity", "identity_accumulate", "none"])
def test_tail_form_is_bitwise_the_dz_form_on_the_masked_gradient(branch):
    rows, C = 37, 16
    gen = torch.Generator(device=DEV).manual_seed(11)
    p, q = _params(C, gen), _params(C, gen)
    y = torch.randn(rows, C, device=DEV, generator=gen) * 0.6 + p.mean
    r = torch.randn(rows, C, device=DEV, generator=gen) * 0.6 + q.mean
    gout = torch.randn(rows, C, device=DEV, generator=gen)
    ds = branch == "downsample"
    has_r = branch != "none"
    out = torch.empty(rows, C, device=DEV)
    _lib.call("dn_bn_add_relu_fwd", y.data_ptr(), p.scale.data_ptr(), p.shift.data_ptr(), r.data_ptr() if has_r else None,
              q.scale.data_ptr() if ds else None, q.shift.data_ptr() if ds else None, rows, C, out.data_ptr(), _stream())
    nblk = _lib.load().dn_reduce_blocks(rows, C)
    before = torch.randn(rows, C, device=DEV, generator=gen)           # what an earlier consumer left in the identity's gradient
    acc = branch == "identity_accumulate"

    def dr_buffer():
        return before.clone() if acc else torch.full((rows, C), float("nan"), device=DEV)

    # A: the train-mode tail writes the masked gradient m (and the identity's share); the dz form turns it into dy / dr
    m = torch.empty(rows, C, device=DEV)
    dr_a = dr_buffer()
    scratch = torch.empty(nblk, C, 4, device=DEV)
    _lib.call("dn_bn_add_relu_bwd", gout.data_ptr(), out.data_ptr(), y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr(),
              r.data_ptr() if has_r else None, q.mean.data_ptr() if ds else None, q.invstd.data_ptr() if ds else None, rows, C, m.data_ptr(),
              dr_a.data_ptr() if has_r else None, int(acc), scratch.data_ptr(), _stream())
    dy_a, part_y = _dz_form(m, y, p)
    if ds:
        dr_a, part_r = _dz_form(m, r, q)
    # B: the frozen tail in one pass
    dy_b = torch.full((rows, C), float("nan"), device=DEV)
    dr_b = dr_buffer()
    part_b = torch.empty(nblk, C, 4, device=DEV)
    _lib.call("dn_bn_frozen_add_relu_bwd", gout.data_ptr(), out.data_ptr(), y.data_ptr(), p.mean.data_ptr(), p.invstd.data_ptr(),
              p.gamma.data_ptr(), r.data_ptr() if has_r else None, q.mean.data_ptr() if ds else None, q.invstd.data_ptr() if ds else None,
              q.gamma.data_ptr() if ds else None, rows, C, dy_b.data_ptr(), dr_b.data_ptr() if has_r else None, int(acc), part_b.data_ptr(),
              _stream())
    dg, db, dbias = _finalize(part_b, p, 4, 0)
    torch.cuda.synchronize()
    assert 0 < int((m == 0).sum()) < m.numel()
    assert torch.equal(dy_a, dy_b)
    assert torch.equal(part_b[:, :, 0:2], part_y)                       # same rows per block, same order: the sums too
    _assert_fp64(dy_b, m, y, p, dg, db, dbias)
    assert torch.equal(dbias, (p.gamma * p.invstd) * db)
    if has_r:
        assert torch.equal(dr_a, dr_b)
    if ds:
        assert torch.equal(part_b[:, :, 2:4], part_r)
        dg_r, db_r, dbias_r = _finalize(part_b, q, 4, 2)
        torch.cuda.synchronize()
        _assert_fp64(dr_b, m, r, q, dg_r, db_r, dbias_r)
    elif has_r:
        assert bool((part_b[:, :, 2:4] == 0).all())
        assert torch.equal(dr_b, before + m if acc else m)


def test_finalize_orders_agree_with_fp64_beyond_the_sliced_range():
    """More partial rows than the sliced order takes (128): the one-block-per-channel order; an odd stride keeps the sliced order out
    too.  Both against fp64 (the rows meet in double precision: one rounding to fp32 at the end, bound u |sum| + tiny)."""
    C = 20
    gen = torch.Generator(device=DEV).manual_seed(3)
    p = _params(C, gen)
    for nrows, stride, offset in ((300, 2, 0), (40, 3, 1), (40, 4, 2)):
        partial = torch.randn(nrows, C, stride, device=DEV, generator=gen)
        dg, db, dbias = _finalize(partial, p, stride, offset)
        torch.cuda.synchronize()
        s0, s1 = partial[:, :, offset].double().sum(0), partial[:, :, offset + 1].double().sum(0)
        assert torch.equal(db, s0.float()) and torch.equal(dg, s1.float()), (nrows, stride, offset)
        assert torch.equal(dbias, (p.gamma * p.invstd) * db)
