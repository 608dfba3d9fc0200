"""GB6m (vector leaves: ops.pack_forest / predict_forest, SparseGBDT.predict(method="rows")) against
tests/forest_ref.py: leaf ids and f32 margins [rows, K] exactly, margins to T ulps of the f64 sum."""
import functools

import numpy as np
import pytest
import torch

import forest_ref as ref
from dmlc_core_amd import _dmlc, ops
from dmlc_core_amd.models import SparseGBDT
from test_gpu_forest import _dev_csr, _forest, _matrix, _pack
from test_gpu_gbdt_multi import _three_classes

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ids(ntrees, depth):  # the rows' end nodes: the leaves play no part
    return ref.walk(*_matrix()[:3], _forest(ntrees, depth), *_matrix()[3:])


def _vector(ntrees, depth, K):
    rng = np.random.default_rng(K)
    return [dict(t, leaf=rng.standard_normal((t["leaf"].size, K)).astype(np.float32))
            for t in _forest(ntrees, depth)]


def _check(csr, want, trees, K):
    leaves = np.stack([tree["leaf"][want[:, t]] for t, tree in enumerate(trees)])  # [T, rows, K]
    m32 = functools.reduce(np.add, leaves, np.zeros(leaves.shape[1:], np.float32))  # in tree order
    partial = np.cumsum(leaves.astype(np.float64), 0)
    m64, top = partial[-1], np.abs(partial).max(0)  # T f32 additions: T ulps of the largest sum
    forest = _pack(trees, *_matrix()[3:])
    leaf, margin = ops.predict_forest(csr, forest, "leaf"), ops.predict_forest(csr, forest)
    assert leaf.dtype == torch.int32 and torch.equal(leaf.cpu(), torch.from_numpy(want))
    assert margin.dtype == torch.float32 and tuple(margin.shape) == (want.shape[0], K) \
        and torch.equal(margin.cpu(), torch.from_numpy(m32))
    assert (np.abs(margin.cpu().numpy() - m64) <= len(trees) * np.spacing(np.float32(top))).all()


@pytest.mark.parametrize("K,ntrees,depth", [(k, t, 6) for k in (1, 2, 3, 5, 16, 17, 32)
                                            for t in (1, 63, 64, 65, 130)] + [(5, 65, 1)])
def test_margins_and_leaves_equal_the_reference(K, ntrees, depth):
    _check(_dev_csr(*_matrix()[:3]), _ids(ntrees, depth), _vector(ntrees, depth, K), K)


def test_operand_shapes():
    off, idx, val, cut_ptr, cut = _matrix()
    trees, whole = _vector(3, 6, 3), _dev_csr(off, idx, val)
    _check(dict(whole, value=None), ref.walk(off, idx, None, trees, cut_ptr, cut), trees, 3)
    part = dict(whole, offset=whole["offset"][5:12])  # offset[0] != 0, rows of R +- 1 and 2 R + 3
    _check(part, _ids(3, 6)[5:11], trees, 3)
    wide = _matrix(wide=True)[:3]  # ids >= 2^32
    _check(_dev_csr(*wide, "u64"), ref.walk(*wide, trees, cut_ptr, cut), trees, 3)
    none = ops.predict_forest(dict(whole, offset=whole["offset"][:1]), _pack(trees, cut_ptr, cut))
    assert none.dtype == torch.float32 and tuple(none.shape) == (0, 3)
    bad = np.where(np.arange(val.size) == off[10] - 1, np.float32(np.nan), val)  # tree 0's root
    bad, small = _dev_csr(off, idx, bad), _pack(_vector(3, 1, 3), cut_ptr, cut)
    with pytest.raises(ValueError, match="NaN"):
        ops.predict_forest(bad, small)
    assert tuple(ops.predict_forest(bad, small, validate=False).shape) == (off.size - 1, 3)


def test_pack_forest_vector_leaves():
    cuts, trees = _matrix()[3:], _vector(3, 6, 5)
    forest, stacked = _pack(trees, *cuts), np.stack([t["leaf"] for t in trees])  # [T, size, K]
    assert forest["outputs"] == 5 and forest["leaf_value"].is_contiguous()
    assert torch.equal(forest["leaf_value"].cpu(), torch.from_numpy(stacked))
    assert set(_pack(_forest(3, 6), *cuts)) == {"node", "trees", "size", "depth"}
    for refused in (trees[:2] + _forest(3, 6)[2:], trees[:2] + _vector(3, 6, 4)[2:],
                    _vector(3, 6, int(_dmlc.gbdt_max_outputs()) + 1)):  # 1-D among 2-D, unequal
        with pytest.raises(ValueError):                                 # K, K out of range
            _pack(refused, *cuts)


def test_model_rows_path_is_one_fused_walk():
    csr = _three_classes()
    model = SparseGBDT(10, objective="softmax", num_outputs=3, max_depth=3).fit(csr, 4)
    rows = model.predict(csr, method="rows")
    assert tuple(rows.shape) == (600, 3) and model._forest()["outputs"] == 3
    assert torch.equal(rows, model.predict(csr, method="levels")) and torch.equal(rows, model.margin)
