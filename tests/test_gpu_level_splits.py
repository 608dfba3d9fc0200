"""GB9 (ops.level_splits, SparseGBDT(split_search="fused")): the fused level search
against grad_histogram -> best_splits, which it must equal bit for bit, and against
the numpy gain table of tests/gbdt_ref.py."""
import numpy as np
import pytest
import torch

import gbdt_ref as ref
from dmlc_core_amd import ops
from dmlc_core_amd.models import SparseGBDT
from test_gpu_gbdt import ROWS, S, _dev, _gradients, _matrix, _ref_binned, _to_dev

pytestmark = pytest.mark.gpu
KEYS = ("feature", "bin", "default_left", "gain")


def _level(binned_np, num_nodes, first_node, g, h):
    """device operands of one level: pos reaches outside the window on both sides"""
    rng = np.random.default_rng(num_nodes + first_node)
    pos = rng.integers(-1, first_node + num_nodes + 3, binned_np["rows"]).astype(np.int32)
    scale = ref.gradient_scale(g, h)
    sums = ref.node_sums(g, h, pos, num_nodes, scale, first_node)
    return [torch.from_numpy(a).cuda() for a in (g, h, pos, sums)], scale, pos


def _two_step(binned, g, h, pos, sums, scale, first_node, *params):
    hist = ops.grad_histogram(binned, g, h, pos, sums.shape[0], scale, first_node)
    return ops.best_splits(hist, sums, binned["cut_ptr"], scale, *params)


@pytest.mark.parametrize("first_node", [0, 31])
@pytest.mark.parametrize("num_nodes", [1, 2, 33, 64])
@pytest.mark.parametrize("nfeat", [1, 65, 300])
def test_equals_histogram_then_best_splits(nfeat, num_nodes, first_node):
    """columns of 0, 1, 63 .. 65, S - 1 and S entries (owned whole, some ending past their
    segment), of S + 1 and 2 S + 3 (spill path; alone with nfeat = 1); 256-cut columns tile
    33 and 64 nodes"""
    binned_np = _ref_binned(nfeat, True, 256)
    binned = _to_dev(binned_np)
    (g, h, pos, sums), scale, _ = _level(binned_np, num_nodes, first_node, *_gradients())
    got = ops.level_splits(binned, g, h, pos, sums, scale, first_node=first_node)
    want = _two_step(binned, g, h, pos, sums, scale, first_node)
    again = ops.level_splits(binned, g, h, pos, sums, scale, first_node=first_node)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        assert torch.equal(got[k], again[k]), k
    assert nfeat == 1 or (got["feature"] >= 0).any()


def test_against_the_gain_table():
    """the criterion of test_gpu_gbdt._check_splits: the returned gain is the table's at the
    returned (feature, bin, side) and no valid candidate lies above it, both within 1e-12 x
    the largest term of the gain"""
    binned_np = _ref_binned(300, True, 256)
    rng = np.random.default_rng(33)
    g = rng.standard_normal(ROWS).astype(np.float32)
    h = rng.random(ROWS).astype(np.float32)
    (dg, dh, dpos, dsums), scale, pos = _level(binned_np, 33, 0, g, h)
    got = {k: v.cpu().numpy() for k, v in
           ops.level_splits(_to_dev(binned_np), dg, dh, dpos, dsums, scale).items()}
    cut_ptr, sums = binned_np["cut_ptr"], dsums.cpu().numpy()
    hist = ref.grad_histogram(binned_np, g, h, pos, 33, scale)
    table = ref.gain_table(hist, sums, cut_ptr, scale)
    tol = 1e-12 * ref.gain_table(hist, sums, cut_ptr, scale, terms=True)
    valid = np.isfinite(table)
    assert (got["feature"] >= 0).all()
    for n in range(33):
        f, d = got["feature"][n], int(got["default_left"][n])
        assert 0 <= got["bin"][n] < cut_ptr[f + 1] - cut_ptr[f]
        b = cut_ptr[f] + got["bin"][n]
        assert valid[n, b, d] and got["gain"][n] > 0
        assert abs(got["gain"][n] - table[n, b, d]) <= tol[n, b, d]
        over = valid[n] & (table[n] - got["gain"][n] > np.where(valid[n], tol[n], 0.0))
        assert not over.any(), (n, got["gain"][n], table[n][over].max())


def test_more_columns_than_the_staged_pointers_and_no_histogram_in_memory():
    """3000 columns of 1 .. 3 entries: a workgroup owns more columns than it stages pointers
    for; at 64 nodes the call allocates far less than the histogram it replaces"""
    nfeat, rows = 3000, 500
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 4, nfeat)
    r = np.concatenate([np.sort(rng.choice(rows, n, replace=False)) for n in lens])
    c = np.repeat(np.arange(nfeat), lens)
    order = np.lexsort((c, r))
    off = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int64)
    csr = _dev(off, c[order].astype(np.int64), rng.integers(0, 5, r.size).astype(np.float32)[order])
    binned = ops.bin_features(csr, ops.feature_cuts(csr, nfeat), nfeat)
    assert S // 3 > 1016 and r.size > S
    g = rng.standard_normal(rows).astype(np.float32)
    h = rng.random(rows).astype(np.float32)
    for num_nodes in (3, 64):
        pos = rng.integers(0, 3, rows).astype(np.int32)
        scale = ref.gradient_scale(g, h)
        dev = [torch.from_numpy(a).cuda()
               for a in (g, h, pos, ref.node_sums(g, h, pos, num_nodes, scale))]
        ops.level_splits(binned, *dev, scale, min_child_weight=0.1)  # warms the workspace
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got = ops.level_splits(binned, *dev, scale, min_child_weight=0.1)
        peak = torch.cuda.max_memory_allocated() - before
        want = _two_step(binned, *dev, scale, 0, 1.0, 0.0, 0.1)
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k
        assert (got["feature"][:3] >= 0).all()
    assert peak < 64 * binned["cut"].numel() * 16 // 4, peak


def test_edges():
    binned_np = _ref_binned(65, True, 256)
    binned = _to_dev(binned_np)
    (g, h, pos, sums), scale, _ = _level(binned_np, 4, 0, *_gradients())
    best = float(ops.level_splits(binned, g, h, pos, sums, scale)["gain"].max())
    assert best > 0
    none = ops.level_splits(binned, g, h, pos, sums, scale, gamma=best + 1.0)
    assert (none["feature"] == -1).all() and not none["gain"].any()
    heavy = ops.level_splits(binned, g, h, pos, sums, scale, min_child_weight=1e4 * ROWS + 1.0)
    assert (heavy["feature"] == -1).all()
    empty = {"offset": torch.zeros(1, dtype=torch.int64).cuda(),
             "index": torch.zeros(0, dtype=torch.int32).cuda(),
             "value": torch.zeros(0, dtype=torch.float32).cuda()}
    zero = torch.zeros(0, dtype=torch.float32).cuda()
    for b, gg, pp in ((ops.bin_features(empty, ops.feature_cuts(empty, 5), 5), zero, zero.int()),
                      (dict(binned, rows=0), zero, zero.int())):
        out = ops.level_splits(b, gg, gg, pp, sums, 1.0)
        assert out["feature"].tolist() == [-1] * 4 and not out["gain"].any()
        assert out["bin"].dtype == torch.int32 and out["default_left"].dtype == torch.bool
    with pytest.raises(ValueError, match="reg_lambda"):
        ops.level_splits(binned, g, h, pos, sums, scale, reg_lambda=0.0)
    with pytest.raises(ValueError, match="node_sum"):
        ops.level_splits(binned, g, h, pos, sums.reshape(-1), scale)
    with pytest.raises(ValueError, match="grad_histogram_multi"):
        ops.level_splits(binned, g.reshape(-1, 1), h.reshape(-1, 1), pos, sums, scale)


def test_model_grows_the_same_trees():
    off, idx, val = _matrix(300, True)
    csr = _dev(off, idx, val)
    csr["label"] = torch.from_numpy((np.random.default_rng(4).random(ROWS) < 0.4)
                                    .astype(np.float32)).cuda()
    fused = SparseGBDT(300, max_depth=4, split_search="fused").fit(csr, 3)
    plain = SparseGBDT(300, max_depth=4).fit(csr, 3)
    assert len(fused.trees) == 3 and (plain.trees[0]["feature"] >= 0).any()
    for a, b in zip(fused.trees, plain.trees):
        for k in ("feature", "bin", "default_left", "leaf"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(fused.predict(csr), plain.predict(csr))
    with pytest.raises(ValueError, match="split_search"):
        SparseGBDT(300, split_search="x")
    with pytest.raises(ValueError, match="fused"):
        SparseGBDT(300, split_search="fused", num_outputs=2)
