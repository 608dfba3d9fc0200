"""FF1 / FF2 (src/gpu/ffm_kernels.hip) through ops.ffm / ops.ffm_t /
ops.csr_ffm and SparseFFM, against the definition evaluated in float64 with
numpy in this file.

Bound, derived as in test_gpu_spmm.py: an output is a sum of T terms
x_a x_b V V -- for p[r] T = pairs * k, for a dV element T = the ordered pairs
that contribute to it -- each term carries at most three product roundings,
and the terms are summed in any order, so

    |got - ref| <= (T + 4) * 2^-23 * sum |term|

with the sum of |term| computed in float64 next to the reference.  No other
tolerance appears in this file, except the 1e-4 the end-to-end test is given.

Row lengths: around the pair-slot counts (2, 3), the wave (63, 64, 65), a long
staged row (the capacity is 128), the first length that is not staged
(capacity + 1), 200, empty rows, and 121 random lengths in 0 .. 40.  FF1 gives
8 rows to a workgroup and FF2 4, so the row count is 133, which neither
divides."""
import functools

import numpy as np
import pytest
import torch

from dmlc_core_amd import _dmlc, data, ops
from dmlc_core_amd.models import SparseFFM

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23
F = 70
CAP = int(_dmlc.ffm_staged_row_entries())
LENS = [0, 1, 2, 3, 63, 64, 65, 200, 0, 17, 0]
LONG_ROW = len(LENS)  # the row of CAP + 1 entries
FIELDS = [1, 5]
RANKS = [4, 8, 16, 32]


@functools.lru_cache(maxsize=None)
def _host(nf, ordered):
    """offset, ids (with duplicates), fields (random, or ascending within every
    row), values"""
    rng = np.random.default_rng(17)
    lens = np.array(LENS + [CAP + 1] + rng.integers(0, 41, 121).tolist(), np.int64)
    assert len(lens) % 8 != 0 and len(lens) % 4 != 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(off[-1])
    idx = rng.integers(0, F, nnz)
    fld = rng.integers(0, nf, nnz)
    if ordered:
        for b, e in zip(off[:-1], off[1:]):
            fld[b:e] = np.sort(fld[b:e])
    val = rng.standard_normal(nnz).astype(np.float32)
    return off, idx, fld, val


@functools.lru_cache(maxsize=None)
def _table(nf, k, feats=F):
    return np.random.default_rng(1000 * nf + k).standard_normal((feats, nf, k)).astype(np.float32)


def _dev_csr(off, idx, fld, val, index64=False):
    it = np.int64 if index64 else np.int32
    return {"offset": torch.from_numpy(np.ascontiguousarray(off)).cuda(),
            "index": torch.from_numpy(idx.astype(it)).cuda(),
            "field": torch.from_numpy(fld.astype(it)).cuda(),
            "value": None if val is None else torch.from_numpy(np.ascontiguousarray(val)).cuda()}


def _row_products(off, idx, fld, val, v, r):
    """of row r: ids i, fields f, xx[a, b] = x_a x_b, va[a, b] = V[i_a, f_b],
    vb[a, b] = V[i_b, f_a], all float64"""
    b, e = int(off[r]), int(off[r + 1])
    i, f = idx[b:e].astype(np.int64), fld[b:e].astype(np.int64)
    x = np.ones(e - b) if val is None else val[b:e].astype(np.float64)
    v = v.astype(np.float64)
    return i, f, np.outer(x, x), v[i[:, None], f[None, :]], v[i[None, :], f[:, None]]


def _forward_ref(off, idx, fld, val, v):
    """p[r], and its bound, for rows off[0] .. off[-1] of the entry arrays"""
    rows, k = len(off) - 1, v.shape[2]
    p, tol = np.zeros(rows), np.zeros(rows)
    for r in range(rows):
        n = int(off[r + 1] - off[r])
        if n < 2:
            continue
        _, _, xx, va, vb = _row_products(off, idx, fld, val, v, r)
        upper = np.triu(np.ones((n, n), bool), 1)
        p[r] = ((xx * (va * vb).sum(-1))[upper]).sum()
        mag = ((np.abs(xx) * np.abs(va * vb).sum(-1))[upper]).sum()
        tol[r] = (n * (n - 1) // 2 * k + 4) * U23 * mag
    return p, tol


def _backward_ref(off, idx, fld, val, v, g):
    """dV, and its bound: T counts the ordered pairs of rows with g != 0"""
    dv, mag, cnt = np.zeros(v.shape), np.zeros(v.shape), np.zeros(v.shape[:2])
    for r in range(len(off) - 1):
        n = int(off[r + 1] - off[r])
        if n < 2 or g[r] == 0:
            continue
        i, f, xx, _, vb = _row_products(off, idx, fld, val, v, r)
        pair = ~np.eye(n, dtype=bool)
        term = float(g[r]) * (xx * pair)[:, :, None] * vb
        where = (np.broadcast_to(i[:, None], (n, n)), np.broadcast_to(f[None, :], (n, n)))
        np.add.at(dv, where, term)
        np.add.at(mag, where, np.abs(term))
        np.add.at(cnt, where, pair.astype(np.float64))
    return dv, (cnt[:, :, None] + 4) * U23 * mag


def _within(got, ref, tol, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= tol)  # a NaN (unwritten output) is bad
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5], tol[bad][:5])


def _variants(nf):
    for ordered in (False, True):
        off, idx, fld, val = _host(nf, ordered)
        for v in (val, None):
            yield ordered, off, idx, fld, v


@pytest.mark.parametrize("index64", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("nf", FIELDS)
def test_ffm_forward_edge_rows(nf, k, index64):
    """all 133 rows, the first 11 through an offset slice, rows 5 .. 59 through
    a slice that does not start at 0; fields random and ascending, value
    present and None; the same bytes from a second call"""
    table = _table(nf, k)
    vd = torch.from_numpy(table).cuda()
    for ordered, off, idx, fld, val in _variants(nf):
        t = _dev_csr(off, idx, fld, val, index64)
        ref, tol = _forward_ref(off, idx, fld, val, table)
        y = ops.ffm(t, vd)
        assert y.dtype == torch.float32 and y.shape == (len(off) - 1,)
        what = (nf, k, index64, ordered, val is not None)
        _within(y, ref, tol, what)
        assert torch.equal(y, ops.ffm(t, vd)), what
        assert torch.equal(y, ops.ffm(t, vd, validate=False)), what
        head = ops.ffm(dict(t, offset=t["offset"][:len(LENS) + 1]), vd)
        _within(head, ref[:len(LENS)], tol[:len(LENS)], what + ("head",))
        sl = dict(t, offset=t["offset"][5:61])
        assert int(sl["offset"][0]) != 0
        _within(ops.ffm(sl, vd), ref[5:60], tol[5:60], what + ("slice",))
        assert not y[[0, 1, 8, 10]].any()  # rows of 0 or 1 entries


def test_ffm_no_rows_and_no_entries():
    off, idx, fld, val = _host(5, False)
    t = _dev_csr(off, idx, fld, val)
    vd = torch.from_numpy(_table(5, 8)).cuda()
    none = ops.ffm(dict(t, offset=t["offset"][:1]), vd)
    assert none.shape == (0,) and none.dtype == torch.float32
    empty = _dev_csr(np.zeros(6, np.int64), idx[:0], fld[:0], val[:0])
    assert torch.equal(ops.ffm(empty, vd), torch.zeros(5, device="cuda"))
    g = torch.ones(0, device="cuda")
    dv = ops.ffm_t(dict(t, offset=t["offset"][:1]), g, vd)
    assert dv.shape == vd.shape and dv.dtype == torch.float32 and not dv.any()
    assert not ops.ffm_t(empty, torch.ones(5, device="cuda"), vd).any()


def _upstream(rows):
    g = np.random.default_rng(23).standard_normal(rows).astype(np.float32)
    g[[2, 7, 20]] = 0.0  # the 3-entry row, the 200-entry row, a random one
    g[5] = -0.0
    return g


@pytest.mark.parametrize("index64", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("nf", FIELDS)
def test_ffm_t_matches_the_definition(nf, k, index64):
    """the gradient for a random upstream g with rows of g == +-0, on all rows
    and on a row slice that does not start at 0"""
    table = _table(nf, k)
    vd = torch.from_numpy(table).cuda()
    for ordered, off, idx, fld, val in _variants(nf):
        t = _dev_csr(off, idx, fld, val, index64)
        g = _upstream(len(off) - 1)
        what = (nf, k, index64, ordered, val is not None)
        dv = ops.ffm_t(t, torch.from_numpy(g).cuda(), vd)
        assert dv.shape == vd.shape and dv.dtype == torch.float32
        ref, tol = _backward_ref(off, idx, fld, val, table, g)
        _within(dv, ref, tol, what)
        sl = dict(t, offset=t["offset"][5:61])
        ref, tol = _backward_ref(off[5:61], idx, fld, val, table, g[5:60])
        _within(ops.ffm_t(sl, torch.from_numpy(g[5:60].copy()).cuda(), vd), ref, tol,
                what + ("slice",))


@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("nf", FIELDS)
def test_csr_ffm_backward_is_ffm_t(nf, k):
    """d/dv of csr_ffm(...).sum() against ffm_t(csr, ones, v): two runs of the
    same atomic sums, each within the bound of the exact value, so within twice
    the bound of each other"""
    table = _table(nf, k)
    off, idx, fld, val = _host(nf, True)
    t = _dev_csr(off, idx, fld, val)
    v = torch.from_numpy(table).cuda().requires_grad_()
    y = ops.csr_ffm(t, v)
    assert torch.equal(y.detach(), ops.ffm(t, v.detach()))
    y.sum().backward()
    ones = np.ones(len(off) - 1, np.float32)
    direct = ops.ffm_t(t, torch.from_numpy(ones).cuda(), v.detach())
    ref, tol = _backward_ref(off, idx, fld, val, table, ones)
    _within(v.grad, direct.cpu().numpy().astype(np.float64), 2 * tol, "autograd vs ffm_t")
    _within(v.grad, ref, tol, "autograd vs definition")


@pytest.mark.parametrize("index64", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("row", [4, LONG_ROW], ids=["staged_row", "long_row"])
@pytest.mark.parametrize("kind", ["id", "field"])
def test_out_of_range_entries_are_reported_and_skipped(kind, row, index64):
    """one entry with id = F (or field = num_fields) in a staged row or in the
    row that is re-read from global memory: ops.ffm raises naming it; with
    validate=False, and in ffm_t, the entry takes part in no pair -- the result
    is the definition's on the CSR without that entry.  The kernels never form
    an address from such an entry."""
    nf, k = 5, 8
    table = _table(nf, k)
    vd = torch.from_numpy(table).cuda()
    off, idx, fld, val = (a.copy() for a in _host(nf, False))
    j = int(off[row]) + 7
    if kind == "id":
        idx[j] = F
    else:
        fld[j] = nf
    t = _dev_csr(off, idx, fld, val, index64)
    with pytest.raises(ValueError, match="feature id is >= F" if kind == "id"
                       else "field is >= num_fields") as info:
        ops.ffm(t, vd)
    assert ("field is" in str(info.value)) == (kind == "field")
    assert ("feature id" in str(info.value)) == (kind == "id")
    with pytest.raises(ValueError):
        ops.csr_ffm(t, vd.clone().requires_grad_())
    # the CSR without entry j
    off2 = off.copy()
    off2[row + 1:] -= 1
    idx2, fld2, val2 = (np.delete(a, j) for a in (idx, fld, val))
    ref, tol = _forward_ref(off2, idx2, fld2, val2, table)
    _within(ops.ffm(t, vd, validate=False), ref, tol, ("skip forward", kind, row))
    g = _upstream(len(off) - 1)
    ref, tol = _backward_ref(off2, idx2, fld2, val2, table, g)
    _within(ops.ffm_t(t, torch.from_numpy(g).cuda(), vd), ref, tol, ("skip backward", kind, row))


def test_ffm_rejects_a_transpose_and_operands_on_the_host():
    off, idx, fld, val = _host(5, False)
    t = _dev_csr(off, idx, fld, val)
    vd = torch.from_numpy(_table(5, 8)).cuda()
    with pytest.raises(ValueError, match="transpose"):
        ops.ffm(ops.transpose(t, F), vd)
    with pytest.raises(ValueError, match="CSR's device"):
        ops.ffm(t, vd.cpu())
    with pytest.raises(ValueError, match="CSR's device"):
        ops.ffm_t(t, torch.ones(len(off) - 1), vd)
    with pytest.raises(ValueError, match="rows"):
        ops.ffm_t(t, torch.ones(3, device="cuda"), vd)
    with pytest.raises(ValueError, match="entries"):
        ops.ffm(dict(t, field=t["field"][:-1]), vd)


def _rel(got, ref):
    """largest difference relative to the reference's largest magnitude"""
    ref = ref.detach().cpu().double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def test_libfm_file_to_sparse_ffm_loss(tmp_path):
    """300 LibFM lines (4 fields, ids < 64, every third row with one field
    repeated) -> GPUParser -> csr_to_torch -> SparseFFM.loss -> backward: the
    loss and the three gradients against the same model on CPU copies of the
    same tensors (SparseFFM.reference), within 1e-4 of the reference's largest
    magnitude; and ops.ffm after ops.gather_rows, bitwise"""
    rng = np.random.default_rng(41)
    nf, feats, rank = 4, 64, 4
    lines = []
    for r in range(300):
        fields = list(range(nf))
        if r % 3 == 0:
            fields += [int(rng.integers(0, nf))] * int(rng.integers(1, 4))
        ents = " ".join("%d:%d:%.4f" % (f, rng.integers(0, feats), rng.standard_normal())
                        for f in sorted(fields))
        lines.append("%d %s" % (rng.integers(0, 2), ents))
    p = tmp_path / "train.libfm"
    p.write_text("\n".join(lines) + "\n")
    csr = data.GPUParser(str(p), format="libfm").parse_all()
    assert csr.rows == 300 and int(csr.max_field) + 1 == nf and int(csr.max_index) < feats
    t = data.csr_to_torch(csr)
    assert t["field"].dtype == t["index"].dtype and t["field"].numel() == t["index"].numel()
    dev = SparseFFM(feats, int(csr.max_field) + 1, rank=rank, seed=1)
    g = torch.Generator().manual_seed(42)
    with torch.no_grad():
        dev.w.copy_(torch.randn(feats, 1, generator=g) * 0.3)
        dev.v.copy_(torch.randn(feats, nf, rank, generator=g) * 0.3)
        dev.bias.fill_(0.1)
    host = SparseFFM(feats, nf, rank=rank, seed=1)
    host.load_state_dict(dev.state_dict())
    dev = dev.cuda()
    cpu = {k: (a.cpu() if isinstance(a, torch.Tensor) else a) for k, a in t.items()}
    for kind in ("logistic", "squared"):
        dev.zero_grad()
        host.zero_grad()
        loss = dev.loss(t, loss=kind)
        loss.backward()
        want = host.loss(cpu, loss=kind)
        want.backward()
        assert _rel(loss, want) <= 1e-4, (kind, float(loss), float(want))
        for name in ("w", "v", "bias"):
            got, ref = getattr(dev, name).grad, getattr(host, name).grad
            assert ref.abs().max() > 0
            assert _rel(got, ref) <= 1e-4, (kind, name, _rel(got, ref))
    sel = torch.from_numpy(rng.permutation(300)[:50].copy()).cuda()
    vd = dev.v.detach()
    every = ops.ffm(t, vd)
    assert torch.equal(ops.ffm(ops.gather_rows(t, sel), vd), every[sel])
