"""GB1 - GB5 (src/gpu/gbdt_kernels.hip) through ops.feature_cuts, bin_features,
grad_histogram, best_splits, advance_rows and models.SparseGBDT, against the
NumPy reference tests/gbdt_ref.py: cuts, bins, histograms and row positions
must equal it exactly, split gains to 1e-12 relative (float64 ulps and FMA
contraction; see _check_splits).

The matrix has 3 S rows (S = _dmlc.gbdt_segment_entries()) and columns of 0, 1,
63, 64, 65, S - 1, S, S + 1 and 2 S + 3 entries among short random ones, so
segments hold many short columns, exactly one column, and pieces of a column
that spans three."""
import functools

import numpy as np
import pytest
import torch

import gbdt_ref as ref
from dmlc_core_amd import _dmlc, ops
from dmlc_core_amd.models import SparseGBDT

pytestmark = pytest.mark.gpu
S = int(_dmlc.gbdt_segment_entries())
ROWS = 3 * S


def _column_values(rng, kind, n):
    """the value content the cuts must get right, by column"""
    if kind == 0:
        return np.full(n, 2.5)                                   # all equal: 1 cut
    if kind == 1:
        return rng.choice([-3.0, 7.0], n)                        # 2 distinct values
    if kind == 2:
        return rng.choice([-0.0, 0.0, 1.0], n)                   # -0.0 is +0.0
    if kind == 3:
        return rng.choice([-np.inf, np.inf, -1.0, 0.5], n)       # infinities are values
    if kind == 4:
        return rng.choice([1e-45, 3e-45, -1e-45, 1e-38, 0.0], n)  # denormals
    if kind == 5:
        return -np.abs(rng.standard_normal(n))                   # negatives
    if kind == 6:
        return rng.permutation(np.arange(n) % 256).astype(np.float64)  # 256 distinct (n >= 256)
    if kind == 7:
        return rng.permutation(np.arange(n) % 257) - 100.0       # 257 distinct (n >= 257)
    return rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def _matrix(nfeat, ends_present):
    """(offset, index, value) of ROWS rows; the first and last feature hold
    entries or are empty, per ``ends_present``"""
    rng = np.random.default_rng(nfeat * 2 + ends_present)
    lengths = np.zeros(nfeat, np.int64)
    kinds = np.full(nfeat, 8)
    if nfeat == 1:
        lengths[0] = 2 * S + 3 if ends_present else 0
        kinds[0] = 7
    else:
        lengths[:] = rng.integers(0, 40, nfeat)
        edge = [0, 1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3]
        where = np.linspace(1, nfeat - 2, len(edge)).astype(int)
        lengths[where] = edge
        kinds[where] = [8, 8, 0, 1, 2, 6, 7, 3, 5]
        short = np.setdiff1d(np.arange(1, nfeat - 1), where)[:8]
        kinds[short] = [0, 1, 2, 3, 4, 5, 4, 2]
        lengths[short] = np.maximum(lengths[short], 5)
        lengths[[0, nfeat - 1]] = [65, S + 1] if ends_present else [0, 0]
        kinds[[0, nfeat - 1]] = [4, 7]
    rows, cols, vals = [], [], []
    for f in range(nfeat):
        n = int(lengths[f])
        rows.append(np.sort(rng.choice(ROWS, n, replace=False)))
        cols.append(np.full(n, f))
        vals.append(_column_values(rng, int(kinds[f]), n))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ROWS))]).astype(np.int64)
    return off, cols[order].astype(np.int64), vals[order].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ref_binned(nfeat, ends_present, max_bins, with_value=True):
    off, idx, val = _matrix(nfeat, ends_present)
    val = val if with_value else None
    cut_ptr, cut = ref.feature_cuts(off, idx, val, nfeat, max_bins)
    return ref.bin_features(off, idx, val, nfeat, cut_ptr, cut)


def _index_tensor(idx, kind):
    if kind == "i64":
        return torch.from_numpy(idx.astype(np.int64))
    if kind == "u64":
        return torch.from_numpy(idx.astype(np.int64)).view(torch.uint64)
    t = torch.from_numpy(idx.astype(np.int32))
    return t.view(torch.uint32) if kind == "u32" else t


def _dev(off, idx, val, kind="i32"):
    return {"offset": torch.from_numpy(np.ascontiguousarray(off)).cuda(),
            "index": _index_tensor(idx, kind).cuda(),
            "value": None if val is None else torch.from_numpy(val).cuda()}


def _same_binned(got, want):
    for k in ("offset", "row", "bin", "cut_ptr", "cut"):
        assert got[k].dtype == torch.from_numpy(want[k]).dtype, k
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    assert got["rows"] == want["rows"]


def _to_dev(binned):
    return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v)
            for k, v in binned.items()}


# ------------------------------------------------------------ cuts and bins
@pytest.mark.parametrize("max_bins", [2, 3, 255, 256])
@pytest.mark.parametrize("ends_present", [True, False])
@pytest.mark.parametrize("nfeat", [1, 65, 300])
def test_cuts_and_bins_equal_the_reference(nfeat, ends_present, max_bins):
    csr = _dev(*_matrix(nfeat, ends_present))
    want = _ref_binned(nfeat, ends_present, max_bins)
    cuts = ops.feature_cuts(csr, nfeat, max_bins)
    assert cuts["cut_ptr"].dtype == torch.int64 and cuts["cut"].dtype == torch.float32
    assert torch.equal(cuts["cut_ptr"].cpu(), torch.from_numpy(want["cut_ptr"]))
    assert torch.equal(cuts["cut"].cpu(), torch.from_numpy(want["cut"]))
    _same_binned(ops.bin_features(csr, cuts, nfeat), want)


@pytest.mark.parametrize("kind", ["u32", "i64", "u64"])
def test_index_widths(kind):
    off, idx, val = _matrix(65, True)
    csr = _dev(off, idx, val, kind)
    _same_binned(ops.bin_features(csr, ops.feature_cuts(csr, 65, 256), 65),
                 _ref_binned(65, True, 256))


def test_without_values_every_entry_is_one():
    off, idx, _ = _matrix(65, True)
    csr = _dev(off, idx, None)
    want = _ref_binned(65, True, 256, with_value=False)
    assert set(want["cut"].tolist()) == {1.0}
    _same_binned(ops.bin_features(csr, ops.feature_cuts(csr, 65, 256), 65), want)


def test_offset_slice():
    off, idx, val = _matrix(65, True)
    whole = _dev(off, idx, val)
    b, e = S // 3, 2 * S + 11
    csr = {"offset": whole["offset"][b:e + 1], "index": whole["index"], "value": whole["value"]}
    assert int(csr["offset"][0]) != 0
    cut_ptr, cut = ref.feature_cuts(off[b:e + 1], idx, val, 65, 255)
    want = ref.bin_features(off[b:e + 1], idx, val, 65, cut_ptr, cut)
    cuts = ops.feature_cuts(csr, 65, 255)
    assert torch.equal(cuts["cut"].cpu(), torch.from_numpy(cut))
    _same_binned(ops.bin_features(csr, cuts, 65), want)


def test_new_data_under_trained_cuts():
    """a value on each cut, just above and below it, below the minimum and above the maximum"""
    nfeat = 65
    trained = _ref_binned(nfeat, True, 256)
    cut_ptr, cut = trained["cut_ptr"], trained["cut"]
    rows, cols, vals = [], [], []
    for f in range(nfeat):
        c = cut[cut_ptr[f]:cut_ptr[f + 1]]
        finite = c[np.isfinite(c)]
        x = np.concatenate([c, np.nextafter(finite, np.float32(np.inf)),
                            np.nextafter(finite, np.float32(-np.inf)),
                            np.float32([-3e38, 3e38, 0.25])])  # an empty feature gets entries too
        vals.append(x.astype(np.float32))
        cols.append(np.full(x.size, f))
        rows.append(np.arange(x.size))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    off = np.concatenate([[0], np.cumsum(np.bincount(rows))]).astype(np.int64)
    idx, val = cols[order].astype(np.int64), vals[order]
    want = ref.bin_features(off, idx, val, nfeat, cut_ptr, cut)
    cuts = {"cut_ptr": torch.from_numpy(cut_ptr).cuda(), "cut": torch.from_numpy(cut).cuda()}
    _same_binned(ops.bin_features(_dev(off, idx, val), cuts, nfeat), want)


def test_nan_and_wide_ids_raise():
    off, idx, val = _matrix(65, True)
    cuts = ops.feature_cuts(_dev(off, idx, val), 65)
    bad = val.copy()
    bad[S + 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ops.feature_cuts(_dev(off, idx, bad), 65)
    with pytest.raises(ValueError, match="NaN"):
        ops.bin_features(_dev(off, idx, bad), cuts, 65)
    bad = -np.abs(val)  # a NaN with the sign bit sorts below -inf
    bad[7] = np.float32(np.nan)
    bad[7:8].view(np.uint32)[:] |= 0x80000000
    with pytest.raises(ValueError, match="NaN"):
        ops.feature_cuts(_dev(off, idx, bad), 65)
    with pytest.raises(ValueError):
        ops.feature_cuts(_dev(off, idx, val), 64)
    with pytest.raises(ValueError):
        ops.bin_features(_dev(off, idx, val), cuts, 64)
    with pytest.raises(ValueError):
        ops.feature_cuts(_dev(off, idx, val), 65, max_bins=257)


# ---------------------------------------------------------------- histogram
def _gradients(seed=5):
    rng = np.random.default_rng(seed)
    g = (rng.choice([-1.0, 1.0], ROWS) * 10.0 ** rng.uniform(-8, 8, ROWS)).astype(np.float32)
    h = (rng.random(ROWS) * 1e4 * (rng.random(ROWS) > 0.1)).astype(np.float32)
    return g, h


@pytest.mark.parametrize("first_node", [0, 31])
@pytest.mark.parametrize("num_nodes", [1, 2, 33, 64])
def test_histogram_equals_the_reference(num_nodes, first_node):
    want_b = _ref_binned(300, True, 256)
    assert np.diff(want_b["cut_ptr"]).max() == 256  # with 64 nodes: more than the LDS table holds
    binned = _to_dev(want_b)
    g, h = _gradients()
    rng = np.random.default_rng(num_nodes + first_node)
    pos = rng.integers(-1, first_node + num_nodes + 3, ROWS).astype(np.int32)
    scale = ops.gradient_scale(torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda())
    assert scale == ref.gradient_scale(g, h)
    args = (binned, torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda(),
            torch.from_numpy(pos).cuda(), num_nodes, scale)
    hist = ops.grad_histogram(*args, first_node=first_node)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (num_nodes, want_b["cut"].size, 2)
    want = ref.grad_histogram(want_b, g, h, pos, num_nodes, scale, first_node)
    assert torch.equal(hist.cpu(), torch.from_numpy(want))
    assert torch.equal(ops.grad_histogram(*args, first_node=first_node), hist)


def test_histogram_of_skipped_rows_and_of_no_rows():
    want_b = _ref_binned(65, True, 256)
    binned = _to_dev(want_b)
    g, h = (torch.from_numpy(a).cuda() for a in _gradients())
    pos = torch.full((ROWS,), -1, dtype=torch.int32).cuda()
    pos[::2] = 9
    hist = ops.grad_histogram(binned, g, h, pos, 4, 2.0 ** 30, first_node=1)
    assert tuple(hist.shape) == (4, want_b["cut"].size, 2) and not hist.any()
    empty = {"offset": torch.zeros(1, dtype=torch.int64).cuda(),
             "index": torch.zeros(0, dtype=torch.int32).cuda(),
             "value": torch.zeros(0, dtype=torch.float32).cuda()}
    cuts = ops.feature_cuts(empty, 5)
    assert cuts["cut_ptr"].tolist() == [0] * 6 and cuts["cut"].numel() == 0
    none = torch.zeros(0, dtype=torch.float32).cuda()
    for c in (cuts, {"cut_ptr": torch.tensor([0, 2, 2, 3, 3, 3]).cuda(),
                     "cut": torch.tensor([1.0, 2.0, 5.0]).cuda()}):
        b = ops.bin_features(empty, c, 5)
        assert b["rows"] == 0 and b["row"].numel() == 0 and b["offset"].tolist() == [0] * 6
        hist = ops.grad_histogram(b, none, none, none.int(), 3, 1.0)
        assert tuple(hist.shape) == (3, c["cut"].numel(), 2) and not hist.any()
    torch.cuda.synchronize()


def test_segment_of_more_columns_than_the_staged_pointers():
    """3000 columns of 1 .. 3 entries: a segment holds over 1016 columns, whose pointers
    do not fit LDS, so the lanes search the column pointer in global memory"""
    nfeat, rows = 3000, 500
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 4, nfeat)
    r = np.concatenate([np.sort(rng.choice(rows, n, replace=False)) for n in lens])
    c = np.repeat(np.arange(nfeat), lens)
    v = rng.integers(0, 5, r.size).astype(np.float32)
    order = np.lexsort((c, r))
    off = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int64)
    idx, val = c[order].astype(np.int64), v[order]
    assert S // 3 > 1016 and idx.size > S
    cut_ptr, cut = ref.feature_cuts(off, idx, val, nfeat)
    want = ref.bin_features(off, idx, val, nfeat, cut_ptr, cut)
    csr = _dev(off, idx, val)
    binned = ops.bin_features(csr, ops.feature_cuts(csr, nfeat), nfeat)
    _same_binned(binned, want)
    g = rng.standard_normal(rows).astype(np.float32)
    h = rng.random(rows).astype(np.float32)
    pos = rng.integers(0, 3, rows).astype(np.int32)
    scale = ref.gradient_scale(g, h)
    hist = ops.grad_histogram(binned, torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda(),
                              torch.from_numpy(pos).cuda(), 3, scale)
    assert torch.equal(hist.cpu(), torch.from_numpy(ref.grad_histogram(want, g, h, pos, 3, scale)))


# ------------------------------------------------------------------- splits
def _check_splits(got, hist, sums, cut_ptr, scale, lam, gamma, mcw):
    """|gain - gain_ref(returned f, t, d)| <= tol and no valid reference
    candidate above the returned gain by more than tol, tol = 1e-12 x the
    largest term of the gain: each term carries a few float64 ulps (2e-16) and
    the device may contract multiplies into FMAs"""
    table = ref.gain_table(hist, sums, cut_ptr, scale, lam, gamma, mcw)
    tol = 1e-12 * ref.gain_table(hist, sums, cut_ptr, scale, lam, gamma, mcw, terms=True)
    feature, tbin = got["feature"].cpu().numpy(), got["bin"].cpu().numpy()
    left, gain = got["default_left"].cpu().numpy(), got["gain"].cpu().numpy()
    assert got["feature"].dtype == torch.int64 and got["bin"].dtype == torch.int32
    assert got["default_left"].dtype == torch.bool and got["gain"].dtype == torch.float64
    valid = np.isfinite(table)
    for n in range(hist.shape[0]):
        if feature[n] < 0:
            returned = 0.0
        else:
            assert cut_ptr[feature[n] + 1] > cut_ptr[feature[n]]  # never a feature without cuts
            assert 0 <= tbin[n] < cut_ptr[feature[n] + 1] - cut_ptr[feature[n]]
            b = cut_ptr[feature[n]] + tbin[n]
            assert valid[n, b, int(left[n])]
            assert abs(gain[n] - table[n, b, int(left[n])]) <= tol[n, b, int(left[n])]
            assert gain[n] > 0
            returned = gain[n]
        over = valid[n] & (table[n] - returned > np.where(valid[n], tol[n], 0.0))
        assert not over.any(), (n, returned, table[n][over].max())


@pytest.mark.parametrize("num_nodes", [1, 33])
def test_best_splits_against_the_gain_table(num_nodes):
    binned = _ref_binned(300, True, 256)
    rng = np.random.default_rng(num_nodes)
    g = rng.standard_normal(ROWS).astype(np.float32)
    h = rng.random(ROWS).astype(np.float32)
    pos = rng.integers(0, num_nodes, ROWS).astype(np.int32)
    scale = ref.gradient_scale(g, h)
    hist = ref.grad_histogram(binned, g, h, pos, num_nodes, scale)
    sums = ref.node_sums(g, h, pos, num_nodes, scale)
    dev = [torch.from_numpy(a).cuda() for a in (hist, sums, binned["cut_ptr"])]
    got = ops.best_splits(*dev, scale, 1.0, 0.0, 1.0)
    assert (got["feature"] >= 0).all()
    _check_splits(got, hist, sums, binned["cut_ptr"], scale, 1.0, 0.0, 1.0)
    again = ops.best_splits(*dev, scale, 1.0, 0.0, 1.0)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    best = float(got["gain"].max())
    none = ops.best_splits(*dev, scale, 1.0, best + 1.0, 1.0)  # gamma above every gain
    assert (none["feature"] == -1).all() and not none["gain"].any()
    _check_splits(none, hist, sums, binned["cut_ptr"], scale, 1.0, best + 1.0, 1.0)
    heavy = ops.best_splits(*dev, scale, 1.0, 0.0, float(ROWS))  # heavier than every child
    assert (heavy["feature"] == -1).all()
    with pytest.raises(ValueError):
        ops.best_splits(*dev, scale, 0.0)


def _tiny(rows_of_features, values, nfeat, g, h):
    """hist, node_sum and cut_ptr of one node over a small dense-ish matrix"""
    lens = [len(r) for r in rows_of_features]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int64) for r in rows_of_features])
    val = np.concatenate([np.asarray(v, np.float32) for v in values])
    cut_ptr, cut = ref.feature_cuts(off, idx, val, nfeat)
    binned = ref.bin_features(off, idx, val, nfeat, cut_ptr, cut)
    g, h = np.asarray(g, np.float32), np.asarray(h, np.float32)
    pos = np.zeros(len(lens), np.int32)
    scale = ref.gradient_scale(g, h)
    return (ref.grad_histogram(binned, g, h, pos, 1, scale), ref.node_sums(g, h, pos, 1, scale),
            cut_ptr, scale)


def test_split_edge_cases():
    # every row in one bin of both features (feature 2 has no cuts): nothing to split
    hist, sums, cut_ptr, scale = _tiny([[0, 1]] * 6, [[4.0, -1.0]] * 6, 3,
                                       [1, -1, 2, -2, 1, 1], [1] * 6)
    got = ops.best_splits(*(torch.from_numpy(a).cuda() for a in (hist, sums, cut_ptr)), scale)
    assert got["feature"].tolist() == [-1] and got["gain"].tolist() == [0.0]
    # feature 1: value 1 with g = +1, value 2 with g = -1; the rows without an
    # entry have g = +1: sending them left separates the signs exactly
    feats = [[1]] * 4 + [[1]] * 4 + [[0]] * 4
    vals = [[1.0]] * 4 + [[2.0]] * 4 + [[3.0]] * 4
    g = [1.0] * 4 + [-1.0] * 4 + [1.0] * 4
    hist, sums, cut_ptr, scale = _tiny(feats, vals, 2, g, [1.0] * 12)
    dev = [torch.from_numpy(a).cuda() for a in (hist, sums, cut_ptr)]
    got = ops.best_splits(*dev, scale)
    want = ref.best_splits(hist, sums, cut_ptr, scale)
    assert want["feature"].tolist() == [1] and want["default_left"].tolist() == [True]
    table = ref.gain_table(hist, sums, cut_ptr, scale)
    assert table[0, 1, 1] > table[0, 1, 0] + 1.0  # strictly better than missing-right
    assert got["feature"].tolist() == [1] and got["bin"].tolist() == [0]
    assert got["default_left"].tolist() == [True]
    _check_splits(got, hist, sums, cut_ptr, scale, 1.0, 0.0, 1.0)
    # no missing rows: both sides tie and missing-right wins; equal gains: the lowest feature
    hist, sums, cut_ptr, scale = _tiny([[0, 1]] * 4, [[1.0, 5.0], [1.0, 5.0], [2.0, 6.0], [2.0, 6.0]],
                                       2, [1, 1, -1, -1], [1] * 4)
    got = ops.best_splits(*(torch.from_numpy(a).cuda() for a in (hist, sums, cut_ptr)), scale)
    assert got["feature"].tolist() == [0] and got["default_left"].tolist() == [False]


# ------------------------------------------------------------------ advance
def _level(binned_np, seed=11):
    """a 4-node window at first_node 3: two nodes split on the column of
    2 S + 3 entries (default right and default left), a leaf, one on a short column"""
    lens = np.diff(binned_np["offset"])
    long_f, short_f = int(np.argmax(lens)), int(np.nonzero(lens == 65)[0][0])
    assert lens[long_f] == 2 * S + 3
    split = {"feature": np.array([long_f, long_f, -1, short_f], np.int64),
             "bin": np.array([100, 3, 0, 0], np.int32),
             "default_left": np.array([False, True, False, True])}
    # ids no row holds yet: rows at 7 and 8, above the window, must not join a child
    left, right = np.array([15, 17, 19, 21], np.int32), np.array([16, 18, 20, 22], np.int32)
    pos = np.random.default_rng(seed).integers(0, 9, ROWS).astype(np.int32)
    return split, left, right, pos


def test_advance_equals_the_reference_and_splits_the_histogram_exactly():
    binned_np = _ref_binned(300, True, 256)
    binned = _to_dev(binned_np)
    split, left, right, pos = _level(binned_np)
    dsplit = {k: torch.from_numpy(v).cuda() for k, v in split.items()}
    dpos = torch.from_numpy(pos).cuda()
    new = ops.advance_rows(binned, dpos, dsplit, torch.from_numpy(left).cuda(),
                           torch.from_numpy(right).cuda(), first_node=3)
    want = ref.advance_rows(binned_np, pos, split, left, right, first_node=3)
    assert new.dtype == torch.int32 and torch.equal(new.cpu(), torch.from_numpy(want))
    assert torch.equal(dpos.cpu(), torch.from_numpy(pos))  # the input is not written
    outside = (pos < 3) | (pos > 6)
    assert np.array_equal(want[outside], pos[outside])
    for n in (0, 1, 3):  # rows without an entry in the split column exist and follow the default
        assert ((pos == 3 + n) & (want == (left[n] if split["default_left"][n] else right[n]))).any()
    g, h = (torch.from_numpy(a).cuda() for a in _gradients())
    scale = ops.gradient_scale(g, h)
    parent = ops.grad_histogram(binned, g, h, dpos, 4, scale, first_node=3)
    child = ops.grad_histogram(binned, g, h, new, 8, scale, first_node=15)
    assert torch.equal(parent, child[0::2] + child[1::2])
    assert parent.any()


# -------------------------------------------------------------------- model
@functools.lru_cache(maxsize=None)
def _table():
    rng = np.random.default_rng(21)
    x = rng.integers(0, 200, (300, 20)).astype(np.float32) / 200
    keep = rng.random(x.shape) < 0.9
    keep[:, 3] = True
    off = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    r, c = np.nonzero(keep)
    return x, off, c.astype(np.int64), x[r, c]


def _table_csr(label):
    x, off, idx, val = _table()
    csr = _dev(off, idx, val)
    csr["label"] = torch.from_numpy(label.astype(np.float32)).cuda()
    return csr


def test_model_finds_the_separating_feature():
    x = _table()[0]
    label = x[:, 3] > 0.37
    model = SparseGBDT(20, max_depth=1, learning_rate=1.0, objective="squared").fit(
        _table_csr(label), 1)
    tree = model.trees[0]
    assert int(tree["feature"][0]) == 3
    thr = float(model.cuts["cut"][int(model.cuts["cut_ptr"][3]) + int(tree["bin"][0])])
    assert x[~label, 3].max() <= thr < x[label, 3].min()


def test_model_loss_descends_and_predict_reproduces_the_margins():
    x = _table()[0]
    rng = np.random.default_rng(22)
    label = x[:, 3] * 2 - x[:, 7] + 0.1 * rng.standard_normal(300)
    csr = _table_csr(label)
    model = SparseGBDT(20, max_depth=4, learning_rate=0.5, objective="squared")
    model.cuts = ops.feature_cuts(csr, 20)
    binned = ops.bin_features(csr, model.cuts, 20)
    losses = [float(model.loss(torch.zeros(300).cuda(), csr["label"]))]
    for _ in range(10):
        margin = model.boost(binned, csr["label"])
        losses.append(float(model.loss(margin, csr["label"])))
    for a, b in zip(losses, losses[1:]):
        assert b <= a * (1 + 1e-6), losses
    assert losses[-1] < 0.5 * losses[0]
    assert len(model.trees) == 10
    assert float((model.predict(csr) - margin).abs().max()) <= 1e-5
    other = dict(binned, rows=299)  # trees and tracked margins belong to 300 rows
    with pytest.raises(ValueError, match="margins"):
        model.boost(other, csr["label"][:299])
    assert len(model.trees) == 10
    logistic = SparseGBDT(20, max_depth=3, objective="logistic").fit(
        _table_csr(x[:, 3] > 0.37), 3)
    p = torch.sigmoid(logistic.predict(_table_csr(x[:, 3] > 0.37)))
    assert ((p > 0.5).cpu().numpy() == (x[:, 3] > 0.37)).all()


def test_model_refuses_a_host_csr():
    _, off, idx, val = _table()
    host = {"offset": torch.from_numpy(off), "index": torch.from_numpy(idx),
            "value": torch.from_numpy(val), "label": torch.zeros(300)}
    model = SparseGBDT(20)
    with pytest.raises(ValueError):
        model.fit(host, 1)
    with pytest.raises(ValueError):
        model.predict(host)
