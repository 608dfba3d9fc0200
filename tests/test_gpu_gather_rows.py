"""ops.gather_rows (G1 / G2, src/gpu/gather_kernels.hip) and data.RowBatches
against a numpy gather of the same arrays: concatenate arr[off[r]:off[r + 1]]
for r in rows.  The op is pure data movement, so every comparison is bitwise
(values through an int32 view: NaN payloads and -0.0 count)."""
import numpy as np
import pytest
import torch

from dmlc_core_amd import _dmlc, data, ops

pytestmark = pytest.mark.gpu

R = _dmlc.csr_gather_run_entries()  # output entries one wave of G2 owns


def make_csr(lengths, seed=0, index_dtype=torch.int32, value=True, field=False, columns=()):
    """a host CSR (numpy) with the given row lengths and its device dict"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz, n = int(off[-1]), len(lengths)
    np_index = np.int32 if index_dtype == torch.int32 else np.int64
    hi = 2 ** 31 - 1 if index_dtype == torch.int32 else 2 ** 62
    host = {"offset": off, "index": rng.integers(0, hi, nnz).astype(np_index)}
    if value:
        bits = rng.integers(-2 ** 31, 2 ** 31 - 1, nnz).astype(np.int32)  # NaNs, infs, denormals
        bits[::7] = np.int32(-2 ** 31)  # -0.0
        host["value"] = bits.view(np.float32)
    if field:
        host["field"] = rng.integers(0, hi, nnz).astype(np_index)
    if "label" in columns:
        host["label"] = rng.standard_normal(n).astype(np.float32)
    if "weight" in columns:
        host["weight"] = rng.random(n).astype(np.float32)
    if "qid" in columns:
        host["qid"] = rng.integers(0, 2 ** 62, n).astype(np.int64)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    dev.setdefault("value", None)
    return host, dev


def bits(a):
    """an array as integers of its item size (bitwise comparison)"""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def np_gather(arr, off, rows):
    parts = [arr[off[r]:off[r + 1]] for r in rows]
    return np.concatenate(parts) if parts else arr[:0]


def check(res, host, rows, off=None):
    """res is the numpy gather of rows `rows` of host (row pointer `off`)"""
    off = host["offset"] if off is None else off
    rows = np.asarray(rows, dtype=np.int64)
    want_off = np.concatenate([[0], np.cumsum(off[rows + 1] - off[rows])]).astype(np.int64)
    assert res["offset"].dtype == torch.int64
    assert np.array_equal(res["offset"].cpu().numpy(), want_off)
    nnz = int(want_off[-1])
    for k in ("index", "value", "field"):
        if host.get(k) is None:
            assert res.get(k) is None
            continue
        assert res[k].numel() == nnz and res[k].is_contiguous()
        assert res[k].dtype == torch.from_numpy(host[k][:0]).dtype
        assert np.array_equal(bits(res[k]), bits(np_gather(host[k], off, rows))), k
    for k in ("label", "weight", "qid"):
        if k in host:
            assert np.array_equal(bits(res[k]), bits(host[k][rows])), k
        else:
            assert k not in res


def dev_rows(rows, dtype=torch.int64):
    return torch.tensor(np.asarray(rows, dtype=np.int64), dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def basic():
    return make_csr(np.random.default_rng(11).integers(0, 71, 300), seed=1)


@pytest.mark.parametrize("sel", ["permutation", "reversed", "duplicates", "single", "empty"])
def test_basic_selections(basic, sel):
    host, dev = basic
    rows = {"permutation": np.random.default_rng(5).permutation(300),
            "reversed": np.arange(299, -1, -1), "duplicates": [5, 5, 5, 0], "single": [123],
            "empty": []}[sel]
    res = ops.gather_rows(dev, dev_rows(rows))
    check(res, host, rows)
    if sel == "empty":
        assert res["offset"].tolist() == [0]
        assert res["index"].numel() == 0 and res["value"].numel() == 0


def test_run_boundaries():
    """row ends exactly on R - 1, R, R + 1 and 2R, one row of 3R + 7 entries
    between one-entry rows, a long row first and another last"""
    want = [2 * R + 5,                    # long first: ends at 2R + 5
            R - 6, 1, 1, R - 1,           # ends at 3R - 1, 3R, 3R + 1, 4R
            1, 1, 1, 3 * R + 7, 1, 1, 1,  # a long row among one-entry rows
            R + 3]                        # long last
    ends = np.cumsum(want)
    assert {3 * R - 1, 3 * R, 3 * R + 1, 4 * R} <= set(ends.tolist())
    order = np.random.default_rng(2).permutation(len(want))  # source row order[i] = wanted row i
    lengths = np.empty(len(want), dtype=np.int64)
    lengths[order] = want
    host, dev = make_csr(lengths, seed=3)
    check(ops.gather_rows(dev, dev_rows(order)), host, order)
    # the same ends without the leading long row: R - 1, R, R + 1, 2R from position 0
    host, dev = make_csr([R - 1, 1, 1, R - 1, 5], seed=4)
    check(ops.gather_rows(dev, dev_rows(range(5))), host, range(5))


def test_empty_rows():
    lengths = [0] * 5 + [3, 70] + [0] * 100 + [9] + [0] * 300 + [R + 1, 2] + [0] * 7
    host, dev = make_csr(lengths, seed=5)
    n = len(lengths)
    check(ops.gather_rows(dev, dev_rows(range(n))), host, range(n))  # start, middle blocks, end
    rev = np.arange(n - 1, -1, -1)
    check(ops.gather_rows(dev, dev_rows(rev)), host, rev)
    only_empty = [0, 1, 2, 8, 9, 10, n - 1] * 20  # 140 empty rows: wider than a wave
    res = ops.gather_rows(dev, dev_rows(only_empty))
    check(res, host, only_empty)
    assert res["offset"].tolist() == [0] * (len(only_empty) + 1) and res["index"].numel() == 0


def test_sliced_source(basic):
    host, dev = basic
    sl = {"offset": dev["offset"][100:201], "index": dev["index"], "value": dev["value"]}
    off = host["offset"][100:201]
    assert off[0] != 0
    rows = np.random.default_rng(8).permutation(100)
    check(ops.gather_rows(sl, dev_rows(rows)), host, rows, off=off)
    with pytest.raises(ValueError, match="nrows"):
        ops.gather_rows(sl, dev_rows([100]))  # a row of the whole CSR, past the slice


@pytest.mark.parametrize("kw", [
    dict(value=False),
    dict(field=True),
    dict(index_dtype=torch.int64, field=True),
    dict(columns=("label", "weight", "qid")),
    dict(columns=("label",)),
], ids=["no-value", "field", "u64", "label-weight-qid", "label"])
@pytest.mark.parametrize("rows_dtype", [torch.int32, torch.int64], ids=["rows32", "rows64"])
def test_columns(kw, rows_dtype):
    lengths = np.random.default_rng(21).integers(0, 50, 200)
    host, dev = make_csr(lengths, seed=6, **kw)
    rows = np.random.default_rng(22).integers(0, 200, 333)
    res = ops.gather_rows(dev, dev_rows(rows, rows_dtype))
    check(res, host, rows)
    if not kw.get("value", True):
        assert "value" in res and res["value"] is None


def test_errors_and_error_word_cleared(basic):
    host, dev = basic
    with pytest.raises(ValueError, match="nrows"):
        ops.gather_rows(dev, dev_rows([3, 300, 4]))
    with pytest.raises(ValueError, match="nrows"):
        ops.gather_rows(dev, dev_rows([3, -1, 4]))
    with pytest.raises(ValueError, match="nrows"):
        ops.gather_rows(dev, dev_rows([-1], torch.int32))
    rows = [7, 299, 0]
    check(ops.gather_rows(dev, dev_rows(rows)), host, rows)
    # with out=: the flagged call has written nothing outside the buffers, the next one is right
    out = ops.gather_rows(dev, dev_rows(range(40)))  # room for what follows
    with pytest.raises(ValueError, match="nrows"):
        ops.gather_rows(dev, dev_rows([1, 300, 2]), out=out)
    check(ops.gather_rows(dev, dev_rows([2, 1, 0]), out=out), host, [2, 1, 0])


def test_out_reuses_buffers(basic):
    host, dev = basic
    a = np.argsort(-np.diff(host["offset"]))[:50]  # the 50 longest rows
    b = np.random.default_rng(9).permutation(300)[:50]
    first = ops.gather_rows(dev, dev_rows(a))
    ptrs = {k: first[k].data_ptr() for k in ("offset", "index", "value")}
    second = ops.gather_rows(dev, dev_rows(b), out=first)
    assert {k: second[k].data_ptr() for k in ptrs} == ptrs
    check(second, host, b)
    fewer = b[:20]  # fewer rows fit too
    third = ops.gather_rows(dev, dev_rows(fewer), out=second)
    assert third["index"].data_ptr() == ptrs["index"]
    check(third, host, fewer)


def test_out_too_small_is_not_overrun(basic):
    host, dev = basic
    rows = np.random.default_rng(10).permutation(300)[:120]
    nnz = int((host["offset"][rows + 1] - host["offset"][rows]).sum())
    # buffers left by a smaller first call
    small = ops.gather_rows(dev, dev_rows(rows[:3]))
    with pytest.raises(ValueError, match="does not fit"):
        ops.gather_rows(dev, dev_rows(rows), out=small)
    # enough rows, too few entries: a larger backing tensor sliced down shows what follows
    for short in (nnz - 1, nnz - R - 3, 0):
        back_i = torch.full((nnz + 256,), -7, dtype=torch.int32, device="cuda")
        back_v = torch.full((nnz + 256,), -7.0, dtype=torch.float32, device="cuda")
        out = {"offset": torch.empty(len(rows) + 1, dtype=torch.int64, device="cuda"),
               "index": back_i[:short], "value": back_v[:short]}
        with pytest.raises(ValueError, match="does not fit"):
            ops.gather_rows(dev, dev_rows(rows), out=out)
        assert bool((back_i[short:] == -7).all()) and bool((back_v[short:] == -7.0).all())
    # the exact size fits
    out = {"offset": torch.empty(len(rows) + 1, dtype=torch.int64, device="cuda"),
           "index": back_i[:nnz], "value": back_v[:nnz]}
    res = ops.gather_rows(dev, dev_rows(rows), out=out)
    check(res, host, rows)
    assert res["index"].data_ptr() == back_i.data_ptr()
    assert bool((back_i[nnz:] == -7).all()) and bool((back_v[nnz:] == -7.0).all())


def test_side_stream_and_determinism(basic):
    host, dev = basic
    rows = np.random.default_rng(12).integers(0, 300, 1000)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        r = dev_rows(rows)
        a = ops.gather_rows(dev, r)
        b = ops.gather_rows(dev, r)
        check(a, host, rows)
        for k in ("offset", "index", "value"):
            assert np.array_equal(bits(a[k]), bits(b[k]))
    torch.cuda.synchronize()


def test_positions_past_2_31():
    """64-bit positions on both sides: source entries past 2^31 of a large
    index array (only its tail is ever written or read), and a batch whose
    output positions pass 2^31 (one long row selected over and over; compared
    on the device, row by row, with the source row)"""
    base = 2 ** 31 + 12345
    lengths = np.array([40, 0, 700, 3], dtype=np.int64)
    off = base + np.concatenate([[0], np.cumsum(lengths)])
    big = torch.empty(int(off[-1]), dtype=torch.int32, device="cuda")  # 8 GiB, not filled
    tail = np.random.default_rng(3).integers(0, 2 ** 31 - 1, int(lengths.sum())).astype(np.int32)
    big[base:] = torch.from_numpy(tail).cuda()
    dev = {"offset": torch.from_numpy(off).cuda(), "index": big, "value": None}
    rows = [2, 0, 3, 1, 2]
    res = ops.gather_rows(dev, dev_rows(rows))
    host = {"offset": off - base, "index": tail}
    check(res, host, rows)
    del big, dev, res
    n_long, times = 2 ** 20, 2 ** 11 + 1  # 2^31 + 2^20 output entries
    row = torch.randint(0, 2 ** 31 - 1, (n_long,), dtype=torch.int32, device="cuda")
    src = {"offset": torch.tensor([0, 5, 5 + n_long], device="cuda"),
           "index": torch.cat([torch.zeros(5, dtype=torch.int32, device="cuda"), row]),
           "value": None}
    res = ops.gather_rows(src, torch.ones(times, dtype=torch.int64, device="cuda"))
    assert res["index"].numel() == times * n_long > 2 ** 31
    assert torch.equal(res["offset"], torch.arange(times + 1, device="cuda") * n_long)
    got = res["index"].view(times, n_long)
    for b in range(0, times, 256):
        assert bool((got[b:b + 256] == row).all()), b


@pytest.fixture(scope="module")
def parsed(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gather") / "s.libsvm")
    data.write_synthetic(p, 0, 3000, seed=1, num_features=5000)
    csr = data.GPUParser(p).parse_all()
    return data.csr_to_torch(csr), csr


def dense_ref(t, nfeat):
    off = t["offset"].cpu().numpy().astype(np.int64)
    idx = t["index"].cpu().numpy().astype(np.int64)
    val = t["value"].cpu().numpy()
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    x = torch.zeros((len(off) - 1, nfeat), dtype=torch.float32)
    x.index_put_((torch.from_numpy(rows), torch.from_numpy(idx)), torch.from_numpy(val),
                 accumulate=True)
    return x


def test_consumers_spmv_and_gradient(parsed):
    t, csr = parsed
    nfeat = int(csr.max_index) + 1
    g = torch.Generator().manual_seed(4)
    rows = torch.randint(0, csr.rows, (1500,), generator=g).cuda()
    w = torch.randn(nfeat, generator=g).cuda()
    batch = ops.gather_rows(t, rows)
    assert batch["label"].numel() == 1500
    assert torch.equal(batch["label"], t["label"][rows])
    torch.testing.assert_close(ops.spmv(batch, w), ops.spmv(t, w)[rows], rtol=1e-5, atol=1e-4)
    # the weight gradient of sum(d * (X_batch w + b)) is X_batch^T d
    d = torch.randn(1500, generator=g).cuda()
    wp = w.clone().requires_grad_(True)
    bias = torch.zeros(1, device="cuda", requires_grad=True)
    (ops.csr_spmv(batch, wp, bias, grad="atomic") * d).sum().backward()
    x = dense_ref(t, nfeat)[rows.cpu()]
    torch.testing.assert_close(wp.grad.cpu(), x.t() @ d.cpu(), rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def labelled():
    """1000 rows; row r has r % 7 entries, all equal to r, and label r"""
    r = np.arange(1000)
    lengths = r % 7
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = np.repeat(r, lengths)
    return {"offset": torch.from_numpy(off).cuda(),
            "index": torch.from_numpy(ids.astype(np.int32)).cuda(),
            "value": torch.from_numpy(ids.astype(np.float32)).cuda(),
            "label": torch.from_numpy(r.astype(np.float32)).cuda()}


def epoch_items(it):
    """one epoch as host copies: (labels, offset, index, value) per batch"""
    return [tuple(b[k].cpu().clone() for k in ("label", "offset", "index", "value")) for b in it]


def assert_entries_match_labels(items):
    for label, offset, index, value in items:
        lab = label.long()
        assert torch.equal(offset, torch.cat([torch.zeros(1, dtype=torch.int64),
                                              torch.cumsum(lab % 7, 0)]))
        want = torch.repeat_interleave(lab, lab % 7)
        assert torch.equal(index.long(), want) and torch.equal(value, want.float())


@pytest.mark.parametrize("seed,epoch", [(0, 0), (3, 2)])
def test_row_batches_follow_row_order(labelled, seed, epoch):
    it = data.RowBatches(labelled, 128, seed=seed)
    it.set_epoch(epoch)
    assert len(it) == 8
    items = epoch_items(it)
    assert [len(i[0]) for i in items] == [128] * 7 + [104]
    labels = torch.cat([i[0] for i in items]).long()
    assert torch.equal(labels, data.row_order(1000, seed, epoch))
    assert_entries_match_labels(items)
    again = torch.cat([i[0] for i in epoch_items(it)]).long()  # the same epoch again
    assert torch.equal(again, labels)
    it.set_epoch(epoch + 1)
    other = torch.cat([i[0] for i in epoch_items(it)]).long()
    assert not torch.equal(other, labels)
    assert torch.equal(other, data.row_order(1000, seed, epoch + 1))


def test_row_batches_file_order_and_drop_last(labelled):
    items = epoch_items(data.RowBatches(labelled, 128, shuffle=False))
    assert torch.equal(torch.cat([i[0] for i in items]).long(), torch.arange(1000))
    assert_entries_match_labels(items)
    items = epoch_items(data.RowBatches(labelled, 128, shuffle=False, drop_last=True))
    assert torch.equal(torch.cat([i[0] for i in items]).long(), torch.arange(896))


def test_row_batches_resume_mid_epoch(labelled):
    a = data.RowBatches(labelled, 128, seed=5)
    a.set_epoch(1)
    ia = iter(a)
    for _ in range(3):
        next(ia)
    state = a.state_dict()
    assert state["next_batch"] == 3 and state["epoch"] == 1
    rest_a = [b["label"].cpu().clone() for b in ia]
    b = data.RowBatches(labelled, 128, seed=5)
    b.load_state_dict(state)
    rest_b = [x["label"].cpu().clone() for x in b]
    assert len(rest_a) == len(rest_b) == 5
    assert all(torch.equal(x, y) for x, y in zip(rest_a, rest_b))
    assert torch.equal(torch.cat(rest_b).long(), data.row_order(1000, 5, 1)[3 * 128:])


def test_row_batches_item_survives_the_next_request(labelled):
    it = iter(data.RowBatches(labelled, 128, seed=1, buffers=2))
    prev = next(it)
    for _ in range(7):
        kept = {k: prev[k].clone() for k in ("label", "offset", "index", "value")}
        cur = next(it)
        torch.cuda.synchronize()
        for k, v in kept.items():  # item k is intact after item k + 1 was requested
            assert torch.equal(prev[k], v), k
        assert cur["index"].data_ptr() != prev["index"].data_ptr()
        prev = cur
