"""The HashedFM kernels (src/gpu/fm_kernels.hip) one by one, through the
bindings, against fp64 of the very operands each kernel consumes.

The tests choose every operand ([w | V] already in bf16, q, g, xv, the fp8
codes), so no operand rounding separates kernel and reference and what is
left is f32 accumulation, whose bound is derived (pyref.fm_forward_ref):
K * 2^-23 * sum |a_k b_k| for a K-term product sum, carried to first order
through the epilogue.  A dropped, doubled or misplaced column or row moves a
result by a whole term, far outside that.  Shapes: every dim path (F1 up to
its LDS limit 2048, F2's second feature slab with inactive waves at 1152 and
1536), row counts around the 32-row tile, and grids in which a wave or a
workgroup takes no tile, one, or several.
"""
import numpy as np
import pytest
import torch

import pyref
from dmlc_core_amd import _dmlc

pytestmark = pytest.mark.gpu
U23, U24 = pyref.U23, pyref.U24
ROWS = [1, 31, 32, 33, 95, 96, 97, 257, 1100]
SX = 1.0 / 32


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _codes(rng, rows, dim):
    """fp8 bytes over all 254 finite codes (+-448 and the subnormals
    included) with zeros mixed in, in an allocation of exactly its size"""
    xb = rng.choice(pyref.E4M3_FINITE, size=(rows, dim)).astype(np.uint8)
    xb[rng.random((rows, dim)) < 0.3] = 0
    xb[0, :4] = [0x7E, 0xFE, 0x01, 0x81]
    return xb, torch.from_numpy(xb).cuda().clone()


def _model(rng, dim):
    """[w | V]^T in bf16 [17, dim] (as f32 values), q and bias chosen by the test"""
    wt = pyref.bf16_round((rng.standard_normal((17, dim)) * 0.05).astype(np.float32))
    q = (rng.random(dim) * 0.04).astype(np.float32)
    return wt, q, 0.3


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _within(got, ref, tol, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= tol)  # a NaN (unwritten output) is bad
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5], tol[bad][:5])


# ------------------------------------------------------------------ F0
@pytest.mark.parametrize("dim", [128, 200, 2048])
def test_f0_prep(dim):
    """wt = bf16([w | V]^T) bit for bit (ties to even included), q = rowsum(V^2)
    within the f32 bound of 16 squares and their sum"""
    rng = np.random.default_rng(dim)
    w = (rng.standard_normal(dim) * 0.05).astype(np.float32)
    v = (rng.standard_normal((dim, 16)) * 0.05).astype(np.float32)
    ties = ((np.arange(0x3C00, 0x3C00 + 32, dtype=np.uint32) << 16) | 0x8000).view(np.float32)
    v[:2] = ties.reshape(2, 16)  # exactly between two bf16 values, both parities
    w[:3] = [ties[0], -ties[1], 0.0]
    wt = torch.zeros((17, dim), dtype=torch.bfloat16, device="cuda")
    q = torch.full((dim,), float("nan"), device="cuda")
    wd, vd = _dev(w), _dev(v)
    _dmlc.fm_prep(wd.data_ptr(), vd.data_ptr(), dim, wt.data_ptr(), q.data_ptr(), _stream())
    want = torch.cat([torch.from_numpy(w)[None], torch.from_numpy(v).t()]).to(torch.bfloat16)
    assert torch.equal(wt.cpu().view(torch.int16), want.contiguous().view(torch.int16))
    np.testing.assert_array_equal(want.float().numpy(), pyref.bf16_round(
        np.concatenate([w[None], v.T])))
    q64 = (v.astype(np.float64) ** 2).sum(1)
    _within(q.cpu().numpy(), q64, 16 * U24 * q64, "q")


# ------------------------------------------------------------------ F1
@pytest.mark.parametrize("dim", [128, 1152, 1536, 1664, 1792, 2048])
def test_f1_forward(dim):
    """y and xv for every row count around the 32-row tile and grids of 1, 3
    and all CUs (a wave takes no tile, one, or several with the prefetch
    running across tiles); dims up to the LDS-resident [w | V] limit"""
    rng = np.random.default_rng(dim)
    wt, q, bias = _model(rng, dim)
    wt_d, q_d = _dev(wt, torch.bfloat16), _dev(q)
    assert torch.equal(wt_d.float().cpu(), torch.from_numpy(wt))
    b_d = torch.full((1,), bias, device="cuda")
    for rows in ROWS:
        xb, x_d = _codes(rng, rows, dim)
        y, xv, y_tol, xv_tol = pyref.fm_forward_ref(xb, wt, q, np.float32(bias), SX)
        for cus in (1, 3, _cus()):
            yk = torch.full((rows,), float("nan"), device="cuda")
            xvk = torch.full((rows, 16), float("nan"), device="cuda")
            _dmlc.fm_forward(x_d.data_ptr(), rows, dim, wt_d.data_ptr(), q_d.data_ptr(),
                             b_d.data_ptr(), SX, yk.data_ptr(), xvk.data_ptr(), cus, _stream())
            _within(yk.cpu().numpy(), y, y_tol, ("y", rows, cus))
            _within(xvk.cpu().numpy(), xv, xv_tol, ("xv", rows, cus))


def test_f1_rejects_dims_outside_its_range():
    t = torch.zeros(1, device="cuda")
    for dim in (0, 64, 192, 2176):
        with pytest.raises(Exception, match="multiple of 128"):
            _dmlc.fm_forward(t.data_ptr(), 1, dim, t.data_ptr(), t.data_ptr(), t.data_ptr(), 1.0,
                             t.data_ptr(), t.data_ptr(), 1, _stream())


# ------------------------------------------------------------------ F2
def _g_and_xv(rng, rows):
    g = (rng.standard_normal(rows) * 0.1).astype(np.float32)
    g[rng.random(rows) < 0.1] = 0.0
    xv = rng.standard_normal((rows, 16)).astype(np.float32)
    return g, xv


@pytest.mark.parametrize("dim", [128, 1024, 1152, 1536, 2048])
def test_f2_backward(dim):
    """the sum over blocks of part, all 18 rows, for 1, 2, 7 and more
    workgroups than 32-row tiles (trailing workgroups with no rows write
    zeros); dims 1152 and 1536 run the second 1024-feature slab with inactive
    waves.  G is rounded exactly as put_g does, so only accumulation is left."""
    rng = np.random.default_rng(dim + 1)
    for rows in ROWS:
        xb, x_d = _codes(rng, rows, dim)
        g, xv = _g_and_xv(rng, rows)
        z, tol = pyref.fm_backward_ref(xb, g, xv)
        g_d, xv_d = _dev(g).clone(), _dev(xv).clone()
        tiles = (rows + 31) // 32
        for nblk in (1, 2, 7, tiles + 3):
            part = torch.full((nblk, 18, dim), float("nan"), device="cuda")
            _dmlc.fm_backward(x_d.data_ptr(), rows, dim, g_d.data_ptr(), xv_d.data_ptr(), nblk,
                              part.data_ptr(), _stream())
            p = part.cpu().numpy().astype(np.float64)
            assert not np.isnan(p).any(), ("unwritten partials", rows, nblk)
            _within(p.sum(0), z, tol, ("part", rows, nblk))
            per = -(-(-(-rows // nblk)) // 32) * 32
            empty = [b for b in range(nblk) if b * per >= rows]
            assert not p[empty].any()


# ------------------------------------------------------------------ F3 / F4
@pytest.mark.parametrize("dim", [128, 200, 1152])
@pytest.mark.parametrize("nblk", [1, 5, 37, 600])
def test_f3_f4_reduce_grads(dim, nblk):
    """dw = s Z_0 and dV = s Z_{1+f} - V s^2 t from random partials, against
    the fp64 formula (test_pyref_numeric.py confirms it against autograd);
    37 and 600 blocks run the 8-deep unrolled loads"""
    rng = np.random.default_rng(dim * 1000 + nblk)
    part = rng.standard_normal((nblk, 18, dim)).astype(np.float32)
    v = (rng.standard_normal((dim, 16)) * 0.05).astype(np.float32)
    sx = np.float32(0.3)
    dw, dv, dw_tol, dv_tol = pyref.fm_grads_ref(part, v, sx)
    p_d, v_d = _dev(part), _dev(v)
    z = torch.full((18, dim), float("nan"), device="cuda")
    gw = torch.full((dim,), float("nan"), device="cuda")
    gv = torch.full((dim, 16), float("nan"), device="cuda")
    _dmlc.fm_reduce_grads(p_d.data_ptr(), nblk, dim, v_d.data_ptr(), float(sx), z.data_ptr(),
                          gw.data_ptr(), gv.data_ptr(), _stream())
    _within(z.cpu().numpy(), part.astype(np.float64).sum(0),
            (nblk + 4) * U24 * np.abs(part.astype(np.float64)).sum(0), "z")
    _within(gw.cpu().numpy(), dw, dw_tol, "dw")
    _within(gv.cpu().numpy(), dv, dv_tol, "dV")


# ------------------------------------------------------------------ F5
def _loss_ref(y, lab, wgt, kind, inv_n):
    """per-row loss and g = dloss/dy * weight / n in fp64 from the kernel's
    own y, with the error the f32 evaluation may add: a few roundings of
    terms of size |y| + 1 (logistic; exp, log and reciprocal are 1-ulp
    hardware functions of values in (0, 2]) or (y - label)^2 (squared)"""
    y = y.astype(np.float64)
    if kind == 1:
        d = y - lab
        l, dl = d * d, 2 * d
        l_err = 8 * U24 * d * d
    else:
        e = np.exp(-np.abs(y))
        l = np.maximum(y, 0) - y * lab + np.log1p(e)
        dl = np.where(y >= 0, 1 / (1 + e), e / (1 + e)) - lab
        l_err = 8 * U24 * (np.abs(y) + 1)
    g = dl * wgt * inv_n
    g_err = 10 * U24 * np.maximum(1.0, np.abs(dl)) * wgt * inv_n
    return l * wgt, l_err * wgt, g, g_err


def _bf16_64(x):
    return pyref.bf16_round(np.asarray(x, np.float32)).astype(np.float64)


def _exact_operands(rng, rows, dim):
    """operands whose x.[w | V] sums are exact in f32 in any order: x from the
    codes that are multiples of 2^-6 with |x| <= 2, [w | V] = k 2^-7 with
    |k| <= 8, so every product is a multiple of 2^-13 and every partial sum
    stays below 2^24 of those units (2048 terms of at most 2^10)"""
    ok = [c for c in pyref.E4M3_FINITE
          if abs(pyref.E4M3[c]) <= 2 and pyref.E4M3[c] * 64 == round(pyref.E4M3[c] * 64)]
    xb = rng.choice(np.array(ok, np.uint8), size=(rows, dim)).astype(np.uint8)
    xb[rng.random((rows, dim)) < 0.3] = 0
    wt = (rng.integers(-8, 9, size=(17, dim)) / 128.0).astype(np.float32)
    assert np.array_equal(pyref.bf16_round(wt), wt)
    assert (np.abs(pyref.E4M3[xb]) @ np.abs(wt).T).max() * 2.0 ** 13 < 2.0 ** 24
    return xb, torch.from_numpy(xb).cuda().clone(), wt


@pytest.mark.parametrize("dim", [128, 256, 512, 1024])
@pytest.mark.parametrize("kind,weighted", [(0, False), (0, True), (1, False), (1, True)])
@pytest.mark.parametrize("operands", ["all_codes", "exact_sums"])
def test_f5_fused_step(dim, kind, weighted, operands):
    """y as F1; the loss and bias-gradient sums and the partials of G^T x,
    with g formed from the kernel's own y.

    The kernel rounds G = [g, g sx xV] to bf16 from its own f32 xV and g,
    which differ from the reference's by their accumulation / evaluation
    error (the fused step does not write xV out).  Where that interval
    straddles a bf16 rounding boundary the element may land one bf16 step
    away, and there the element's |x| times that step is added to the bound.
    With all 254 codes the K * 2^-23 bound on xV is, from a few hundred
    features on, as wide as a bf16 step, so that allowance dominates; the
    "exact_sums" operands make every x.[w | V] sum exact in f32 in any order
    (xV carries no error), which leaves only g's few ulps: there a few
    elements in a hundred get any allowance and the bound is F2's."""
    rng = np.random.default_rng(dim * 10 + kind * 2 + weighted)
    exact = operands == "exact_sums"
    sx = 1.0 if exact else SX
    wt, q, bias = _model(rng, dim)
    q_d = _dev(q)
    b_d = torch.full((1,), bias, device="cuda")
    for rows in (1, 31, 33, 97, 200):
        if exact:
            xb, x_d, wt = _exact_operands(rng, rows, dim)
        else:
            xb, x_d = _codes(rng, rows, dim)
        wt_d = _dev(wt, torch.bfloat16)
        x = pyref.E4M3[xb]
        lab = (rng.random(rows) > 0.5).astype(np.float32)
        wgt = (rng.random(rows) + 0.5).astype(np.float32) if weighted else np.ones(rows, np.float32)
        lab_d = _dev(lab)
        w_d = _dev(wgt) if weighted else None
        y, xv, y_tol, xv_tol = pyref.fm_forward_ref(xb, wt, q, np.float32(bias), sx)
        if exact:
            xv_tol = np.zeros_like(xv_tol)  # sx = 1 and exact sums: the kernel's xV is xv
        inv_n = np.float32(1.0 / rows)
        tiles = (rows + 31) // 32
        for nblk in (1, 5, tiles + 2):
            yk = torch.full((rows,), float("nan"), device="cuda")
            part = torch.full((nblk, 18, dim), float("nan"), device="cuda")
            lpart = torch.full((nblk, 2), float("nan"), device="cuda")
            _dmlc.fm_fused(x_d.data_ptr(), rows, dim, wt_d.data_ptr(), q_d.data_ptr(),
                           b_d.data_ptr(), sx, lab_d.data_ptr(),
                           0 if w_d is None else w_d.data_ptr(), kind, float(inv_n), nblk,
                           yk.data_ptr(), part.data_ptr(), lpart.data_ptr(), _stream())
            yk = yk.cpu().numpy()
            _within(yk, y, y_tol, ("y", rows, nblk))
            l, l_err, g, g_err = _loss_ref(yk, lab.astype(np.float64), wgt.astype(np.float64),
                                           kind, float(inv_n))
            lp = lpart.cpu().numpy().astype(np.float64).sum(0)
            _within(lp[0:1], l.sum(keepdims=True),
                    l_err.sum(keepdims=True) + (rows + 4) * U24 * np.abs(l).sum(keepdims=True), "loss")
            _within(lp[1:2], g.sum(keepdims=True),
                    g_err.sum(keepdims=True) + (rows + 4) * U24 * np.abs(g).sum(keepdims=True), "sum g")
            # G as the kernel forms it: bf16(g), bf16((g * sx) * xV_unscaled)
            u = np.concatenate([g[:, None], g[:, None] * xv], axis=1)
            du = np.concatenate([g_err[:, None],
                                 g_err[:, None] * np.abs(xv) + np.abs(g)[:, None] * xv_tol
                                 + 4 * U24 * np.abs(g[:, None] * xv)], axis=1)
            gm = _bf16_64(u)
            step = np.maximum(np.abs(_bf16_64(u + du) - gm), np.abs(gm - _bf16_64(u - du)))
            z = np.concatenate([gm.T @ x, g[None, :] @ (x * x)], axis=0)
            tol = rows * U23 * np.concatenate([np.abs(gm).T @ np.abs(x),
                                               np.abs(g)[None, :] @ (x * x)], axis=0)
            tol += np.concatenate([step.T @ np.abs(x), g_err[None, :] @ (x * x)], axis=0)
            p = part.cpu().numpy().astype(np.float64)
            assert not np.isnan(p).any(), ("unwritten partials", rows, nblk)
            _within(p.sum(0), z, tol, ("part", rows, nblk))


def test_f5_rejects_other_dims():
    t = torch.zeros(1, device="cuda")
    for dim in (0, 64, 384, 2048):
        with pytest.raises(Exception, match="128, 256, 512 or 1024"):
            _dmlc.fm_fused(t.data_ptr(), 1, dim, t.data_ptr(), t.data_ptr(), t.data_ptr(), 1.0,
                           t.data_ptr(), 0, 0, 1.0, 1, t.data_ptr(), t.data_ptr(), t.data_ptr(),
                           _stream())
