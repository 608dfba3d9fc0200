"""The NumPy reference of the histogram-GBDT ops (tests/gbdt_ref.py) against
hand cases and brute force; no GPU."""
from fractions import Fraction

import numpy as np
import pytest

import gbdt_ref as ref


def _one_column(values):
    """a CSR of len(values) rows with one entry each, all of feature 0"""
    n = len(values)
    return np.arange(n + 1, dtype=np.int64), np.zeros(n, np.int64), np.asarray(values, np.float32)


@pytest.mark.parametrize("n,want", [(1, 1), (3, 3), (256, 256), (257, 256), (1000, 256)])
def test_cut_counts_of_distinct_values(n, want):
    off, idx, val = _one_column(np.random.default_rng(n).permutation(n))
    cut_ptr, cut = ref.feature_cuts(off, idx, val, 1, 256)
    assert cut_ptr.tolist() == [0, want] and cut.size == want
    assert cut[-1] == val.max() and np.all(np.diff(cut) > 0)
    if n <= 256:
        assert np.array_equal(cut, np.sort(val))


def test_four_bins_of_a_thousand():
    off, idx, val = _one_column(np.random.default_rng(0).permutation(1000))
    cut_ptr, cut = ref.feature_cuts(off, idx, val, 1, 4)
    assert cut.tolist() == [249.0, 499.0, 749.0, 999.0]
    b = ref.bin_features(off, idx, val, 1, cut_ptr, cut)
    assert np.bincount(b["bin"]).tolist() == [250, 250, 250, 250]


def test_zeros_and_infinities():
    off, idx, val = _one_column([-0.0, 0.0, 1, 1, 1, np.inf, -np.inf])
    cut_ptr, cut = ref.feature_cuts(off, idx, val, 1, 256)
    assert cut.tolist() == [-np.inf, 0.0, 1.0, np.inf]
    b = ref.bin_features(off, idx, val, 1, cut_ptr, cut)
    assert b["bin"].tolist() == [1, 1, 2, 2, 2, 3, 0]
    assert b["row"].tolist() == list(range(7))


def test_empty_features_missing_values_and_nan():
    # rows: {1: 2.0}, {}, {1: 2.0, 3: -1.0}; features 0 and 2 are empty, F = 5
    off = np.array([0, 1, 1, 3], np.int64)
    idx = np.array([1, 1, 3], np.int64)
    val = np.array([2.0, 2.0, -1.0], np.float32)
    cut_ptr, cut = ref.feature_cuts(off, idx, val, 5)
    assert cut_ptr.tolist() == [0, 0, 1, 1, 2, 2] and cut.tolist() == [2.0, -1.0]
    cut_ptr1, cut1 = ref.feature_cuts(off, idx, None, 5)  # no values: every entry is 1.0
    assert cut_ptr1.tolist() == cut_ptr.tolist() and cut1.tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        ref.feature_cuts(off, idx, np.array([2.0, np.nan, 1.0], np.float32), 5)
    with pytest.raises(ValueError):
        ref.feature_cuts(off, idx, val, 3)


@pytest.mark.parametrize("max_bins", [2, 3, 255, 256])
def test_last_cut_is_the_maximum(max_bins):
    rng = np.random.default_rng(max_bins)
    for n in (1, 2, max_bins - 1, max_bins, max_bins + 1, 5 * max_bins + 7):
        off, idx, val = _one_column(rng.standard_normal(n).round(1))
        cut_ptr, cut = ref.feature_cuts(off, idx, val, 1, max_bins)
        assert cut[-1] == val.max() and cut.size <= max_bins
        b = ref.bin_features(off, idx, val, 1, cut_ptr, cut)["bin"]
        assert b.max() == cut.size - 1  # the maximum sits in the last bin


def test_new_data_under_trained_cuts():
    cut_ptr, cut = np.array([0, 3], np.int64), np.array([1.0, 2.0, 4.0], np.float32)
    x = np.float32([0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, 3.0, 4.0, 9.0])
    off, idx, val = _one_column(x)
    assert ref.bin_features(off, idx, val, 1, cut_ptr, cut)["bin"].tolist() == [0, 0, 1, 1, 2, 2, 2]


def _problem(rows=400, feats=7, seed=0, density=0.6):
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, feats)) < density
    mask[:, feats - 1] = False  # an empty feature
    dense = rng.integers(0, 9, (rows, feats)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    r, c = np.nonzero(mask)
    return off, c.astype(np.int64), dense[r, c], mask, dense


def test_histogram_matches_float_sums_within_the_rounding_bound():
    rows, feats = 400, 7
    off, idx, val, mask, dense = _problem(rows, feats)
    rng = np.random.default_rng(1)
    g = (rng.standard_normal(rows) * 10.0 ** rng.uniform(-8, 8, rows)).astype(np.float32)
    h = (rng.random(rows) * 1e4).astype(np.float32)
    pos = rng.integers(-1, 4, rows).astype(np.int32)
    cut_ptr, cut = ref.feature_cuts(off, idx, val, feats)
    binned = ref.bin_features(off, idx, val, feats, cut_ptr, cut)
    scale = ref.gradient_scale(g, h)
    s = max(np.abs(g.astype(np.float64)).sum(), np.abs(h.astype(np.float64)).sum())
    assert 2.0 ** 60 < s * scale <= 2.0 ** 61
    qsum = max(np.abs(ref.quantise(g, scale)).astype(object).sum(),
               np.abs(ref.quantise(h, scale)).astype(object).sum())
    assert qsum < 2 ** 62
    hist = ref.grad_histogram(binned, g, h, pos, 3, scale)
    # the brute-force sums of the float64 values, formed exactly (as fractions), so that
    # the only error left is the quantisation's: at most 0.5 / scale per row
    want = np.full(hist.shape, Fraction(0), dtype=object)
    for r in range(rows):
        if not 0 <= pos[r] < 3:
            continue
        for f in np.nonzero(mask[r])[0]:
            c = cut[cut_ptr[f]:cut_ptr[f + 1]]
            b = min(int((c < dense[r, f]).sum()), c.size - 1)
            want[pos[r], cut_ptr[f] + b, 0] += Fraction(float(g[r]))
            want[pos[r], cut_ptr[f] + b, 1] += Fraction(float(h[r]))
    bound = Fraction(rows) / 2 / Fraction(scale)
    assert hist.any()
    for cell, q in np.ndenumerate(hist):
        assert abs(Fraction(int(q)) / Fraction(scale) - want[cell]) <= bound, cell
    # integer sums: a parent is exactly the sum of any partition of its rows
    part = ref.grad_histogram(binned, g, h, np.where(pos == 1, 0, -1).astype(np.int32), 1, scale)
    assert np.array_equal(part[0], hist[1])


def test_gradient_scale_edges():
    assert ref.gradient_scale(np.zeros(3), np.zeros(3)) == 1.0
    assert ref.gradient_scale(np.float32([1.0]), np.float32([0.5])) == 2.0 ** 61
    assert ref.gradient_scale(np.float32([1.5]), np.float32([0.5])) == 2.0 ** 60
    assert ref.gradient_scale(np.float32([0.5, 0.5, 1.0]), np.float32([3.0])) == 2.0 ** 59


@pytest.mark.parametrize("mcw,gamma", [(1.0, 0.0), (0.0, 0.0), (30.0, 0.0), (1.0, 2.0)])
def test_vectorised_split_search_agrees_with_brute_force(mcw, gamma):
    rows, feats = 300, 6
    off, idx, val, _, _ = _problem(rows, feats, seed=3, density=0.5)
    rng = np.random.default_rng(4)
    g = rng.standard_normal(rows).astype(np.float32)
    h = rng.random(rows).astype(np.float32)
    pos = rng.integers(0, 5, rows).astype(np.int32)  # node 4 is outside the window
    cut_ptr, cut = ref.feature_cuts(off, idx, val, feats, 8)
    binned = ref.bin_features(off, idx, val, feats, cut_ptr, cut)
    scale = ref.gradient_scale(g, h)
    hist = ref.grad_histogram(binned, g, h, pos, 4, scale)
    sums = ref.node_sums(g, h, pos, 4, scale)
    a = ref.best_splits(hist, sums, cut_ptr, scale, 1.0, gamma, mcw)
    b = ref.best_splits_brute(hist, sums, cut_ptr, scale, 1.0, gamma, mcw)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.all(a["gain"][a["feature"] >= 0] > 0) and np.all(a["gain"][a["feature"] < 0] == 0)
    assert np.all(a["feature"] != feats - 1)  # the feature without cuts


def test_advance_follows_bins_and_default_sides():
    # feature 0: rows 0, 1, 2 with bins 0, 1, 2; rows 3, 4 have no entry there
    binned = {"offset": np.array([0, 3], np.int64), "row": np.array([0, 1, 2], np.int32),
              "bin": np.array([0, 1, 2], np.uint8), "cut_ptr": np.array([0, 3], np.int64),
              "cut": np.float32([1, 2, 3]), "rows": 5}
    pos = np.array([0, 0, 0, 0, 7], np.int32)
    left, right = np.array([1], np.int32), np.array([2], np.int32)
    for dl, miss in ((False, 2), (True, 1)):
        split = {"feature": np.array([0]), "bin": np.array([1], np.int32),
                 "default_left": np.array([dl])}
        assert ref.advance_rows(binned, pos, split, left, right).tolist() == [1, 1, 2, miss, 7]
    leaf = {"feature": np.array([-1]), "bin": np.array([0], np.int32),
            "default_left": np.array([False])}
    assert ref.advance_rows(binned, pos, leaf, left, right).tolist() == [1, 1, 1, 1, 7]
