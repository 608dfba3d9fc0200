"""tests/weighted_cuts_ref.py against the unweighted reference tests/gbdt_ref.py:
unit weights give its cuts, integer weights those of the rows written out."""
import numpy as np
import pytest

import gbdt_ref
import weighted_cuts_ref as wref


def _random_csr(rng, rows, feats):
    lengths = rng.integers(0, feats + 1, rows)
    idx = np.concatenate([np.sort(rng.choice(feats, n, replace=False)) for n in lengths])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    val = rng.choice(np.float32([-2.0, -0.0, 0.0, 0.5, 3.0, np.inf]), idx.size)
    val = np.where(rng.random(idx.size) < 0.5, rng.standard_normal(idx.size), val)
    return off, idx.astype(np.int64), val.astype(np.float32)


@pytest.mark.parametrize("max_bins", [2, 3, 16, 256])
@pytest.mark.parametrize("rows", [1, 7, 300, 1000])
def test_unit_and_integer_weights(rows, max_bins):
    rng = np.random.default_rng(rows + max_bins)
    off, idx, val = _random_csr(rng, rows, 6)
    want = gbdt_ref.feature_cuts(off, idx, val, 6, max_bins)
    got = wref.feature_cuts(off, idx, val, 6, max_bins, np.ones(rows, np.float32))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    k = rng.integers(0, 4, rows)
    keep = np.repeat(np.arange(rows), k)  # row r written k[r] times
    roff = np.concatenate([[0], np.cumsum(np.diff(off)[keep])]).astype(np.int64)
    take = np.concatenate([np.arange(off[r], off[r + 1]) for r in keep] + [np.zeros(0, np.int64)])
    want = gbdt_ref.feature_cuts(roff, idx[take], val[take], 6, max_bins)
    got = wref.feature_cuts(off, idx, val, 6, max_bins, k.astype(np.float32))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
