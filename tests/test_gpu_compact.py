"""U1 - U4 (src/gpu/compact_kernels.hip) through ops.compact_features, against
torch.unique(sorted=True, return_inverse=True) on the host copy of the rows'
entries: ``ids`` and ``index`` must match it exactly.

Shapes sit at the 64-bit bitmap word and at the scan's 2048-word tile (131 072
features per tile): ids 0 and F-1, bit 63 of a word and bit 0 of the next, the
last word of a scan tile and the first word of the next; every batch has more
entries than one 256-thread workgroup."""
import numpy as np
import pytest
import torch

from dmlc_core_amd import ops

pytestmark = pytest.mark.gpu
TILE = 131072  # features per scan tile: 2048 words of 64 bits
FEATURES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
U23 = 2.0 ** -23


def _edge_ids(nf):
    """the ids the module docstring lists, those below nf"""
    want = [0, nf - 1, 63, 64, 127, 128, TILE - 64, TILE - 1, TILE, TILE + 63, TILE + 64,
            2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE, 3 * TILE + 4]
    return np.unique([i for i in want if 0 <= i < nf]).astype(np.int64)


def _host(nf, rows=300, seed=0, extra=900):
    """offset, ids: the edge ids (each at least once) among `extra` random ones,
    shuffled, in rows of random length with some empty"""
    rng = np.random.default_rng(seed + nf)
    idx = np.concatenate([_edge_ids(nf), rng.integers(0, nf, extra)])
    rng.shuffle(idx)
    cuts = np.sort(rng.integers(0, idx.size + 1, rows - 1))
    off = np.concatenate([[0], cuts, [idx.size]]).astype(np.int64)
    return off, idx


def _index_tensor(idx, kind):
    if kind == "i64":
        return torch.from_numpy(idx.astype(np.int64))
    if kind == "u64":
        return torch.from_numpy(idx.astype(np.uint64).view(np.int64)).view(torch.uint64)
    t = torch.from_numpy(idx.astype(np.uint32).view(np.int32))  # the same 4 bytes
    return t.view(torch.uint32) if kind == "u32" else t


def _dev(off, idx, kind="i32", value=True, field=None, seed=1):
    g = torch.Generator().manual_seed(seed)
    csr = {"offset": torch.from_numpy(np.ascontiguousarray(off)).cuda(),
           "index": _index_tensor(idx, kind).cuda(),
           "value": torch.randn(idx.size, generator=g).cuda() if value else None}
    if field is not None:
        csr["field"] = _index_tensor(field, kind).cuda()
    return csr


def _oracle(off, idx):
    lo, hi = int(off[0]), int(off[-1])
    ids, inv = torch.unique(torch.from_numpy(idx[lo:hi].astype(np.int64)), sorted=True,
                            return_inverse=True)
    return ids, inv, torch.from_numpy(off - lo)


def _check(batch, off, idx):
    ids, inv, roff = _oracle(off, idx)
    assert batch["ids"].dtype == torch.int64 and batch["index"].dtype == torch.int32
    assert batch["offset"].dtype == torch.int64
    assert torch.equal(batch["ids"].cpu(), ids)
    assert torch.equal(batch["index"].cpu().long(), inv)
    assert torch.equal(batch["offset"].cpu(), roff)
    assert batch["num_features"] == ids.numel()
    assert not ops._whole(batch)  # "auto" keeps the atomic gradient for a batch made per step
    return batch


@pytest.mark.parametrize("kind", ["i32", "u32", "i64", "u64"])
@pytest.mark.parametrize("nf", FEATURES)
def test_ids_and_slots_match_torch_unique(nf, kind):
    off, idx = _host(nf)
    csr = _dev(off, idx, kind)
    b = _check(ops.compact_features(csr, nf), off, idx)
    assert set(_edge_ids(nf).tolist()) <= set(b["ids"].tolist())
    assert torch.equal(b["value"], csr["value"]) and "field" not in b


def test_one_shared_id_all_distinct_and_one_hot_id():
    nf = TILE + 1
    rows = 400
    off = np.arange(0, 3 * rows + 1, 3, dtype=np.int64)
    same = np.full(3 * rows, TILE - 1, np.int64)
    b = _check(ops.compact_features(_dev(off, same), nf), off, same)
    assert b["ids"].tolist() == [TILE - 1] and not b["index"].any()
    distinct = np.random.default_rng(2).permutation(nf)[:3 * rows].astype(np.int64)
    b = _check(ops.compact_features(_dev(off, distinct), nf), off, distinct)
    assert b["num_features"] == 3 * rows
    hot = distinct.copy()
    hot[::3] = 64  # one id in every row, distinct others
    b = _check(ops.compact_features(_dev(off, hot), nf), off, hot)
    assert b["num_features"] == 2 * rows + 1 - int(64 in distinct[np.arange(3 * rows) % 3 != 0])


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_no_value_and_a_field_column(kind):
    nf = 65
    off, idx = _host(nf, rows=40, extra=500)
    fld = (idx % 7).astype(np.int64)
    csr = _dev(off, idx, kind, value=False, field=fld)
    csr["label"] = torch.arange(40, dtype=torch.float32).cuda()
    csr["qid"] = torch.arange(40).cuda()
    b = _check(ops.compact_features(csr, nf), off, idx)
    assert b["value"] is None
    assert b["field"].dtype == torch.int32 and b["field"].cpu().tolist() == fld.tolist()
    assert b["label"] is csr["label"] and b["qid"] is csr["qid"] and "weight" not in b
    none = ops.compact_features(dict(csr, field=None), nf)
    assert "field" in none and none["field"] is None


def test_a_transposes_pair_views():
    nf = 200
    off, idx = _host(nf, rows=70, extra=600)
    t = ops.transpose(_dev(off, idx), nf)
    assert ops._paired(t)
    toff, tidx = t["offset"].cpu().numpy(), t["index"].cpu().numpy().astype(np.int64)
    b = _check(ops.compact_features(t, 70), toff, tidx)
    assert torch.equal(b["value"], t["value"].contiguous())


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_a_row_slice_marks_only_its_own_entries(kind):
    nf = 3 * TILE + 5
    off, idx = _host(nf, rows=60, extra=700)
    lo, hi = int(off[20]), int(off[41])
    assert 0 < lo < hi < idx.size
    # outside the slice: ids that occur nowhere inside it (the edge ids too)
    inside = set(idx[lo:hi].tolist())
    outside = np.array([i for i in range(TILE - 600, TILE + 600) if i not in inside], np.int64)
    idx[:lo] = outside[:lo]
    idx[hi:] = outside[-(idx.size - hi):]
    fld = (idx % 5).astype(np.int64)
    csr = _dev(off, idx, kind, field=fld)
    sl = dict(csr, offset=csr["offset"][20:42])
    b = _check(ops.compact_features(sl, nf), off[20:42], idx)
    assert not set(b["ids"].tolist()) & set(outside.tolist())
    assert torch.equal(b["value"], csr["value"][lo:hi])
    assert b["field"].cpu().tolist() == fld[lo:hi].tolist()


def test_empty_batches_launch_nothing():
    dev = torch.device("cuda")
    for off in ([0], [0, 0, 0, 0], [5, 5, 5]):
        csr = {"offset": torch.tensor(off, device=dev),
               "index": torch.arange(9, dtype=torch.int32, device=dev),
               "value": torch.ones(9, device=dev), "field": None}
        b = ops.compact_features(csr, 50)
        assert b["num_features"] == 0 and b["ids"].numel() == 0 and b["ids"].dtype == torch.int64
        assert b["index"].numel() == 0 and b["index"].dtype == torch.int32
        assert b["offset"].tolist() == [0] * len(off) and b["value"].numel() == 0
        assert b["field"] is None
        assert ops.spmv(b, torch.zeros(0, device=dev)).tolist() == [0.0] * (len(off) - 1)


def test_a_second_call_sees_none_of_the_firsts_bits():
    """the stale-bitmap test: two calls on one stream, disjoint id sets"""
    nf = TILE + 65
    rng = np.random.default_rng(3)
    off = np.arange(0, 1201, 4, dtype=np.int64)
    even = 2 * rng.integers(0, nf // 2, 1200)
    odd = 2 * rng.integers(0, nf // 2, 1200) + 1
    first = ops.compact_features(_dev(off, even), nf)
    second = ops.compact_features(_dev(off, odd), nf)
    _check(second, off, odd)
    _check(first, off, even)
    assert not set(first["ids"].tolist()) & set(second["ids"].tolist())
    # and a smaller feature space after a larger one, through the same workspace
    small = np.array([0, 63, 64, 3] * 100, np.int64)
    _check(ops.compact_features(_dev(off[:101], small), 65), off[:101], small)


def test_the_same_input_gives_the_same_bytes():
    nf = 3 * TILE + 5
    off, idx = _host(nf, rows=500, extra=20000)
    csr = _dev(off, idx)
    a, b = ops.compact_features(csr, nf), ops.compact_features(csr, nf)
    for k in ("ids", "index", "offset"):
        assert torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr()


@pytest.mark.parametrize("kind,bad", [("i32", 64), ("i32", 2 ** 32 - 1), ("i64", 64),
                                      ("i64", 2 ** 32 - 1), ("i64", 2 ** 40), ("u64", 2 ** 64 - 1)])
def test_an_id_out_of_range_raises_and_forms_no_address(kind, bad):
    nf = 64
    off, idx = _host(nf, rows=30, extra=400)
    idx = idx.astype(np.uint64)
    idx[137] = bad
    csr = _dev(off, idx, kind)
    with pytest.raises(ValueError, match="feature id is >= num_features"):
        ops.compact_features(csr, nf)
    # validate=False: the flagged entry gets slot 0, the others their slots
    b = ops.compact_features(csr, nf, validate=False)
    keep = np.ones(idx.size, bool)
    keep[137] = False
    ids, inv = torch.unique(torch.from_numpy(idx[keep].astype(np.int64)), sorted=True,
                            return_inverse=True)
    assert torch.equal(b["ids"].cpu(), ids)
    assert torch.equal(b["index"].cpu().long()[torch.from_numpy(keep)], inv)
    assert int(b["index"][137]) == 0
    # the next call is clean again
    idx[137] = 5
    _check(ops.compact_features(_dev(off, idx.astype(np.int64), kind), nf), off,
           idx.astype(np.int64))
    # nothing but bad ids: no id to index, so it raises whatever validate says
    allbad = np.full(idx.size, bad, np.uint64)
    with pytest.raises(ValueError, match="feature id is >= num_features"):
        ops.compact_features(_dev(off, allbad, kind), nf, validate=False)


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_spmv_round_trip(kind):
    nf = TILE + 1
    g = torch.Generator().manual_seed(4)
    w = torch.randn(nf, generator=g).cuda()
    # at most one entry per row: a single term, so bit for bit
    rows = 700
    lens = np.random.default_rng(5).integers(0, 2, rows)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.random.default_rng(6).integers(0, nf, int(off[-1]))
    csr = _dev(off, idx, kind)
    b = _check(ops.compact_features(csr, nf), off, idx)
    assert torch.equal(ops.spmv(b, w[b["ids"]]), ops.spmv(csr, w))
    # longer rows: the tolerance of test_gpu_ops.py's spmv against torch
    off, idx = _host(nf, rows=300, extra=5000)
    csr = _dev(off, idx, kind)
    b = _check(ops.compact_features(csr, nf), off, idx)
    got, want = ops.spmv(b, w[b["ids"]], 0.5), ops.spmv(csr, w, 0.5)
    print("spmv round trip: max |diff|", float((got - want).abs().max()))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-4)
    # and the compact gradient is the touched rows of the dense one
    d = torch.randn(300, generator=g).cuda()
    gu, gd = ops.spmv_t(b, d, b["num_features"]), ops.spmv_t(csr, d, nf)
    torch.testing.assert_close(gu, gd[b["ids"]], rtol=1e-4, atol=1e-4)  # test_gpu_ops.py's spmv_t
    untouched = torch.ones(nf, dtype=torch.bool)
    untouched[b["ids"].cpu()] = False
    assert not gd.cpu()[untouched].any()


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_ffm_round_trip(kind):
    """test_gpu_ffm.py's bound: |got - ref| <= (T + 4) * 2^-23 * sum |term| with
    T = pairs * k terms per row, the sum of |term| in float64"""
    nf, nfields, k, rows = 300, 5, 4, 90
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 13, rows)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, nf, int(off[-1]))
    fld = rng.integers(0, nfields, int(off[-1]))
    csr = _dev(off, idx, kind, field=fld)
    v = torch.randn(nf, nfields, k, generator=torch.Generator().manual_seed(9))
    b = _check(ops.compact_features(csr, nf), off, idx)
    vd = v.cuda()
    got, whole = ops.ffm(b, vd[b["ids"]].contiguous()), ops.ffm(csr, vd)
    x, v64 = csr["value"].cpu().double().numpy(), v.double().numpy()
    ref, tol = np.zeros(rows), np.zeros(rows)
    for r in range(rows):
        lo, n = int(off[r]), int(lens[r])
        for a_ in range(n):
            for c_ in range(a_ + 1, n):
                a, c = lo + a_, lo + c_
                prod = v64[idx[a], fld[c]] * v64[idx[c], fld[a]]
                ref[r] += x[a] * x[c] * prod.sum()
                tol[r] += abs(x[a] * x[c]) * np.abs(prod).sum()
        tol[r] *= (n * (n - 1) // 2 * k + 4) * U23
    err = np.abs(got.cpu().double().numpy() - ref)
    print("ffm round trip: max |batch - ref|", err.max(), "max |batch - whole|",
          float((got - whole).abs().max()))
    assert (err <= tol).all()
    assert (np.abs((got - whole).cpu().double().numpy()) <= tol).all()
